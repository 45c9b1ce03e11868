"""Marginals of a conditioned state (``qsv_marginals_cond``): the exact host reference, the group and fix sets the host
and the GPU tests share, and the stand-in engine of the host tests.  TEST INFRASTRUCTURE ONLY; written from the contract
in include/qsv.h.

  marginals_reference   (list of arrays, mass): per group the 2^k sums of p over the matching global indices whose group
                        bits spell the bin (bin bit b <-> group[b]), each bin one ``math.fsum``; ``hi`` is the global index
                        of p[0] (a shard's p: hi = shard << L)
  FIX_SETS, GROUP_SETS  the 14-qubit cases of tests/test_gpu_marginals.py
  CASES                 (name, bits of p, hi, groups, fixed): every planted mistake of tests/test_marginals_model.py fails
                        at least one of them
  MarginalsNumpyEngine  ``CondNumpyEngine`` plus ``marginals_cond`` by the reference, with the entry point's refusals
"""
from __future__ import annotations

import math

import numpy as np

from _post_select_cases import CondNumpyEngine

SUM_SLACK = 2.5e-13        # the engine's sums against fsum (the bound of _sampler_reference's docstring); relative to the bin:
#                            every term is non-negative
MAX_GROUPS, MAX_K, MAX_BINS = 64, 8, 4096


def mask_of(fixed):
    return sum(1 << q for q in fixed), sum(int(v) << q for q, v in fixed.items())


def marginals_reference(p, groups, fix_mask, fix_val, hi=0):
    p = np.asarray(p, dtype=np.float64)
    g = np.arange(p.size, dtype=np.uint64) + np.uint64(hi)
    sel = np.flatnonzero((g & np.uint64(fix_mask)) == np.uint64(fix_val))
    pm, gm = p[sel], g[sel]
    mass = math.fsum(pm.tolist())
    out = []
    for grp in groups:
        j = np.zeros(gm.size, dtype=np.int64)
        for b, q in enumerate(grp):
            j |= ((gm >> np.uint64(q)) & np.uint64(1)).astype(np.int64) << b
        order = np.argsort(j, kind="stable")
        js, ps = j[order], pm[order]
        bins = np.zeros(1 << len(grp), dtype=np.float64)
        edges = np.searchsorted(js, np.arange((1 << len(grp)) + 1))
        for b in range(1 << len(grp)):
            if edges[b + 1] > edges[b]:
                bins[b] = math.fsum(ps[edges[b]:edges[b + 1]].tolist())
        out.append(bins)
    return out, mass


def contradicting_bins(grp, fixed):
    """mask over the bins of a group: True where the bin disagrees with a fixed qubit of the group"""
    j = np.arange(1 << len(grp))
    bad = np.zeros(j.size, dtype=bool)
    for b, q in enumerate(grp):
        if q in fixed:
            bad |= ((j >> b) & 1) != int(fixed[q])
    return bad


# ---- the 14-qubit sets of the GPU tests --------------------------------------------------------------------------------------
N = 14
F11 = {q: (q * 5 + 1) % 3 % 2 for q in range(11)}                      # 8 matching entries: bits 11, 12, 13 free
ALL14 = {q: (0b10110011010101 >> q) & 1 for q in range(N)}              # one entry
FIX_SETS = {
    "contiguous_blocks": {12: 0, 13: 1},
    "strided": {0: 1, 3: 0, 5: 1},
    "mixed": {2: 1, 7: 0, 13: 1},
    "less_than_a_row": F11,
    "one_entry": ALL14,
    "none": {},
}


def _rand_groups(n_groups, ks, seed, n=N):
    rs = np.random.RandomState(seed)
    return [[int(q) for q in rs.choice(n, size=ks[i % len(ks)], replace=False)] for i in range(n_groups)]


GROUP_SETS = {
    "pairs": [[q, q + 1] for q in range(N - 1)],                                    # 13 overlapping pairs
    "mixed_k": [[], [6], [13, 0, 7], [1, 12, 3, 9, 5, 11, 8, 2], [4], []],         # k = 0, 1, 3, 8
    "with_fixed": [[13, 12, 0], [3, 4, 5], [2, 7], [10, 13], [0, 1, 2, 3, 4, 5, 6, 7]],   # every fix set above fixes some of these
    "64_groups": _rand_groups(64, [2, 3, 1, 4, 2, 5], 7),
    "4096_bins": _rand_groups(16, [8], 8),                                          # 16 x 2^8
}
assert sum(1 << len(g) for g in GROUP_SETS["4096_bins"]) == MAX_BINS and len(GROUP_SETS["64_groups"]) == MAX_GROUPS


# ---- the cases that tell the planted mistakes apart ---------------------------------------------------------------------------
# (name, bits of p, hi, groups, fixed)
CASES = [
    ("asymmetric_pair", 6, 0, [[1, 4]], {}),                             # bit order inside a group
    ("k1_then_k2_then_k1", 6, 0, [[0], [2, 5], [3]], {}),                # the offset of group g is not g * 2^k_0; groups follow each other
    ("fixed_elsewhere", 6, 0, [[0, 1]], {4: 1, 5: 0}),                   # fix_val
    ("fixed_in_group", 6, 0, [[4, 2]], {4: 1}),                          # contradicting bins are 0
    ("shard_bit_in_group", 5, 2 << 5, [[6, 1], [5]], {}),                # p is shard 2 of L = 5: qubits 5, 6 come from hi
    ("shard_bit_fixed", 5, 3 << 5, [[0, 6]], {5: 1, 2: 0}),
    ("two_equal_groups", 6, 0, [[3, 1], [3, 1]], {0: 1}),
    ("empty_group", 6, 0, [[], [2]], {1: 0}),
]


# ---- the stand-in engine ------------------------------------------------------------------------------------------------------
class MarginalsNumpyEngine(CondNumpyEngine):
    """CondNumpyEngine with ``marginals_cond`` by the reference; refuses what the entry point refuses (ValueError)"""

    def marginals_cond(self, groups, fix_mask=0, fix_val=0):
        groups = [[int(q) for q in g] for g in groups]
        if not 1 <= len(groups) <= MAX_GROUPS:
            raise ValueError("%d groups, 1..%d supported" % (len(groups), MAX_GROUPS))
        for i, g in enumerate(groups):
            if len(g) > MAX_K:
                raise ValueError("group %d has %d qubits" % (i, len(g)))
            if any(q < 0 or q >= self.n_qubits for q in g):
                raise ValueError("group %d: qubit out of range" % i)
            if len(set(g)) != len(g):
                raise ValueError("group %d: qubit repeated" % i)
        if sum(1 << len(g) for g in groups) > MAX_BINS:
            raise ValueError("more than %d bins" % MAX_BINS)
        if fix_val & ~fix_mask or fix_mask >> self.n_qubits:
            raise ValueError("bad mask")
        owned = sorted(self.sh)
        assert owned == list(range(self.world)), "one process"
        p = np.concatenate([np.abs(self.sh[s]) ** 2 for s in owned])
        self.marginal_calls = getattr(self, "marginal_calls", 0) + 1
        return marginals_reference(p, groups, fix_mask, fix_val)


def factory(n, devices=(0,), rank=None, world_size=None):
    return MarginalsNumpyEngine(n, len(devices))
