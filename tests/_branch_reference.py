"""Numpy reference of the two slot primitives of the level-wise trajectory walk (qsv_branch_mass, qsv_branch_split),
written from their contract in include/qsv.h.  TEST INFRASTRUCTURE ONLY.

A slot is the aligned block of 2^w amplitudes from b << w of a single-shard state.
  branch_mass   per slot the two sums of |amp|^2 by the value of bit ``qubit``, accumulated in longdouble
  branch_split  slot c of the destination <- slot parent[c] of the source projected on bit ``qubit`` == outcome[c], the kept
                amplitudes bit for bit (release: an outcome 1 is stored at bit 0), everything else zero
"""
import numpy as np

from oracle.sharded_numpy import NumpyEngine


def split_array(src, n_dst, w, parent, outcome, qubit, release):
    """the destination vector (n_dst amplitudes) of a split of the vector ``src``"""
    dst = np.zeros(n_dst, dtype=np.complex128)
    i = np.arange(1 << w)
    bit = (i >> qubit) & 1
    for c, (p, o) in enumerate(zip(parent, outcome)):
        blk = np.asarray(src[int(p) << w: (int(p) + 1) << w])
        out = dst[c << w: (c + 1) << w]
        if release and o == 1:
            out[bit == 0] = blk[bit == 1]                    # i -> i | 1 << qubit keeps the order
        else:
            out[bit == o] = blk[bit == o]
    return dst


def mass_array(vec, w, n_slots, qubit):
    """(n_slots, 2) longdouble sums of the vector ``vec``"""
    v = np.asarray(vec[: n_slots << w]).reshape(n_slots, 1 << w)
    p = v.real.astype(np.longdouble) ** 2 + v.imag.astype(np.longdouble) ** 2
    bit = (np.arange(1 << w) >> qubit) & 1
    return np.stack([p[:, bit == 0].sum(axis=1), p[:, bit == 1].sum(axis=1)], axis=1)


class BranchNumpyEngine(NumpyEngine):
    def branch_mass(self, w, n_slots, qubit):
        assert self.world == 1 and 0 <= qubit < w <= self.n_qubits and 1 <= n_slots <= 1 << (self.n_qubits - w)
        return mass_array(self.sh[0], w, n_slots, qubit).astype(np.float64)

    def branch_split(self, src, w, parent, outcome, qubit, release):
        assert src is not self and self.world == 1 and src.world == 1 and 0 <= qubit < w
        assert 1 <= len(parent) == len(outcome) <= 1 << (self.n_qubits - w)
        assert all(0 <= int(p) < 1 << (src.n_qubits - w) for p in parent) and all(int(o) in (0, 1) for o in outcome)
        self.sh[0][:] = split_array(src.sh[0], 1 << self.n_qubits, w, parent, outcome, qubit, release)


def factory(n, devices=(0,), **kw):
    """``engine_factory`` of qcmrf_amd.trajectory.run_trajectories / QsvBackend._engine_factory"""
    return BranchNumpyEngine(n, 1)


def replay_draws(trace, seed, last_level, leaf_draws=True):
    """Replays ``RandomState(seed)`` over the recorded (shots, mass) vectors of a levels walk: every recorded k1 must come out
    again.  A batch whose children are leaves (level + 1 == last_level) is followed by one seed draw per child, in order.
    Returns the number of leaves."""
    rng = np.random.RandomState(seed % (2 ** 32))
    n_leaves = 0
    for level, bits, ks, m0, m1, k1 in trace:
        ks, m0, m1, k1 = np.asarray(ks, dtype=np.int64), np.asarray(m0), np.asarray(m1), np.asarray(k1, dtype=np.int64)
        got = rng.binomial(ks, np.clip(m1 / (m0 + m1), 0.0, 1.0))
        assert np.array_equal(np.asarray(got, dtype=np.int64).reshape(-1), k1), (level, got, k1)
        if level + 1 == last_level:
            n = int(((ks - k1) > 0).sum() + (k1 > 0).sum())
            n_leaves += n
            if leaf_draws:
                for _ in range(n):
                    rng.randint(0, 2 ** 31 - 1)
    return n_leaves


def check_tree(trace, segs, shots):
    """distribution-free invariants of a recorded walk: every node holds a shot, the children's shots are the parent's, the
    nodes of level L + 1 are exactly the children of level L with shots, every level's shots sum to ``shots``"""
    by_level = {}
    for level, bits, ks, m0, m1, k1 in trace:
        assert len(bits) == len(ks) == len(m0) == len(m1) == len(k1) >= 1
        assert all(k >= 1 for k in ks) and all(0 <= b <= k for b, k in zip(k1, ks))
        by_level.setdefault(level, []).extend(zip(bits, ks, k1))
    for level in sorted(by_level):
        nodes = by_level[level]
        assert sum(k for _, k, _ in nodes) == shots, level
        if level + 1 in by_level:
            c = segs[level].measure_clbit
            kids = [(b | (o << c), kk) for b, k, k1 in nodes for o, kk in ((0, k - k1), (1, k1)) if kk]
            assert sorted(kids) == sorted((b, k) for b, k, _ in by_level[level + 1]), level
    return {level: len(v) for level, v in by_level.items()}
