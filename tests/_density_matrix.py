"""Numpy references for noisy runs (test infrastructure).

All read the same ``qsv_op`` records (``program.encode``) that ``qsv_noisy_sample`` consumes:

  density_distribution   exact as a DISTRIBUTION: rho -> U rho U^dg per gate, rho -> sum_p P(p) P rho P^dg per Pauli op,
                         then the distribution over the recorded classical words with the readout flips applied.
                         Counts are held to it by a chi^2 test; it says nothing about a single shot.
  NoisyNumpyEngine       oracle.sharded_numpy.NumpyEngine plus ``noisy_sample``: one trajectory per shot, all shots of a
                         call evolved side by side (the backend's noisy path on a CPU).  Distributional only: its random
                         numbers are numpy's, so its words are not the engine's.  A stand-in backend for host tests.
  _philox_reference.exact_noisy_sample   exact PER SHOT: the same walk with the engine's documented Philox-4x32-10 draws,
                         so it predicts every output word of a call (test_gpu_noise_exact.py holds the kernel to it).

Pauli index p on error qubits j: x bit p >> 2j & 1, z bit p >> 2j+1 & 1 (qcmrf_amd.noise).
"""
from __future__ import annotations

import numpy as np

from oracle.sharded_numpy import NumpyEngine
from qcmrf_amd import _lib


def _records(rec, data):
    for r in rec:
        n = int(r["n"])
        yield (int(r["kind"]), int(r["target"]), [int(x) for x in r["qubits"][:n]], [int(x) for x in r["vals"][:n]],
               int(r["data_off"]), int(r["mask"]), float(r["angle"]))


_PARITY = (np.unpackbits(np.arange(1 << 13, dtype=">u2").view(np.uint8).reshape(-1, 2), axis=1).sum(axis=1) & 1).astype(np.int64)


def _match(idx, qubits, vals):
    ok = np.ones(idx.shape, dtype=bool)
    for q, v in zip(qubits, vals):
        ok &= ((idx >> q) & 1) == v
    return ok


def _tensor(M):
    """(2^W, K) -> (2,)*W + (K,) view: qubit q on axis W-1-q"""
    W = M.shape[0].bit_length() - 1
    return M.reshape((2,) * W + (M.shape[1] if M.ndim > 1 else 1,)), W


def _sl(W, fixed):
    s = [slice(None)] * (W + 1)
    for q, v in fixed.items():
        s[W - 1 - q] = v
    return tuple(s)


def _pauli_rows(M, qubits, p):
    """rows of M times the Pauli with index p on ``qubits`` (new[i ^ x] = old[i] (-1)^|i & z| i^ny)"""
    x = z = ny = 0
    for j, q in enumerate(qubits):
        xb, zb = (p >> (2 * j)) & 1, (p >> (2 * j + 1)) & 1
        x |= xb << q
        z |= zb << q
        ny += xb & zb
    idx = np.arange(M.shape[0])
    ph = (1j ** ny) * (1 - 2 * _PARITY[idx & z])
    A = (M * ph.reshape((-1,) + (1,) * (M.ndim - 1))).reshape(M.shape[0], -1)
    T, W = _tensor(A)
    axes = tuple(W - 1 - q for q in range(W) if (x >> q) & 1)
    return np.ascontiguousarray(np.flip(T, axis=axes) if axes else T).reshape(M.shape)


def _gate_rows(M, kind, t, qs, vs, off, mask, angle, data):
    """the unitary of one record on the rows (axis 0) of M (2-d; updated in place where it can be)"""
    N = M.shape[0]
    T, W = _tensor(M)
    fixed = dict(zip(qs, vs))
    if kind in (_lib.OP_1Q, _lib.OP_MCX):
        s0, s1 = _sl(W, {**fixed, t: 0}), _sl(W, {**fixed, t: 1})
        a0, a1 = T[s0].copy(), T[s1].copy()
        if kind == _lib.OP_MCX:
            T[s0], T[s1] = a1, a0
        else:
            m = data[off:off + 8].view(np.complex128).reshape(2, 2)
            T[s0] = m[0, 0] * a0 + m[0, 1] * a1
            T[s1] = m[1, 0] * a0 + m[1, 1] * a1
        return M
    if kind == _lib.OP_DIAG:
        idx = np.arange(N)
        tab = data[off:off + (2 << len(qs))].view(np.complex128)
        j = np.zeros(N, dtype=np.int64)
        for b, q in enumerate(qs):
            j |= ((idx >> q) & 1) << b
        M *= tab[j][:, None]
        return M
    if kind == _lib.OP_MCPHASE:
        T[_sl(W, fixed)] *= np.exp(1j * angle)
        return M
    raise ValueError("record kind %d has no numpy reference" % kind)


def _pauli_channel(rho, qs, probs):
    """sum_p probs[p] P rho P^dg: for each X part x, rho with the x qubits flipped on both sides times
    G_x[i, j] = sum_z probs[x, z] (-1)^(z . (i xor j)) on the error qubits (the phases of Y cancel)"""
    N = rho.shape[0]
    W = N.bit_length() - 1
    n = len(qs)
    R = rho.reshape((2,) * (2 * W))
    axes = [W - 1 - q for q in qs] + [2 * W - 1 - q for q in qs]
    order = np.argsort(axes)
    shape = [1] * (2 * W)
    for a in axes:
        shape[a] = 2
    out = np.zeros_like(R)
    bits = np.indices((2,) * (2 * n)).reshape(2 * n, -1).T          # (row bits of qs..., col bits of qs...)
    for x in range(1 << n):
        G = np.zeros(1 << (2 * n))
        for z in range(1 << n):
            p = sum((((x >> j) & 1) << (2 * j)) | (((z >> j) & 1) << (2 * j + 1)) for j in range(n))
            if probs[p] == 0:
                continue
            par = np.zeros(len(bits), dtype=np.int64)
            for j in range(n):
                if (z >> j) & 1:
                    par ^= bits[:, j] ^ bits[:, n + j]
            G += probs[p] * (1 - 2 * par)
        if not G.any():
            continue
        Gb = G.reshape((2,) * (2 * n)).transpose(order).reshape(shape)
        flip = tuple(a for j, q in enumerate(qs) if (x >> j) & 1 for a in (W - 1 - q, 2 * W - 1 - q))
        out += (np.flip(R, axis=flip) if flip else R) * Gb
    return out.reshape(N, N)


def _init_vector(N, kind, mask):
    v = np.zeros(N, dtype=np.complex128)
    m = 0 if kind == _lib.OP_INIT_ZERO else mask
    idx = np.arange(N)
    v[(idx & ~m) == 0] = 2.0 ** (-0.5 * bin(m).count("1"))
    return v


def _pauli_probs(data, off, n):
    cum = np.asarray(data[off:off + 4 ** n], dtype=np.float64)
    return np.diff(np.concatenate([[0.0], cum]))


def word_distribution(p_basis, meas_qubits, readout=None):
    """basis-state distribution -> distribution over the recorded words (bit j = qubit meas_qubits[j], -1: 0), then each
    bit j flipped with readout[j][value]"""
    nb = len(meas_qubits)
    idx = np.arange(p_basis.size)
    w = np.zeros(p_basis.size, dtype=np.int64)
    for j, q in enumerate(meas_qubits):
        if q >= 0:
            w |= ((idx >> q) & 1) << j
    dist = np.bincount(w, weights=p_basis, minlength=1 << nb).astype(np.float64)
    if readout is not None:
        words = np.arange(1 << nb)
        for j, q in enumerate(meas_qubits):
            if q < 0:
                continue
            f0, f1 = float(readout[j][0]), float(readout[j][1])
            bit = (words >> j) & 1
            stay = np.where(bit == 0, 1.0 - f0, 1.0 - f1)
            new = dist * stay
            np.add.at(new, words ^ (1 << j), dist * (1.0 - stay))
            dist = new
    return dist


def density_distribution(rec, data, n_qubits, meas_qubits, readout=None):
    """exact distribution of the recorded words of a noisy program (density matrix of 2^W x 2^W)"""
    N = 1 << n_qubits
    rho = np.zeros((N, N), dtype=np.complex128)
    rho[0, 0] = 1.0
    data = np.ascontiguousarray(data, dtype=np.float64)
    for kind, t, qs, vs, off, mask, angle in _records(rec, data):
        if kind in (_lib.OP_INIT_ZERO, _lib.OP_INIT_UNIFORM):
            v = _init_vector(N, kind, mask)
            rho = np.outer(v, v.conj())
        elif kind == _lib.OP_PAULI:
            rho = _pauli_channel(rho, qs, _pauli_probs(data, off, len(qs)))
        else:
            a = _gate_rows(rho.copy(), kind, t, qs, vs, off, mask, angle, data)
            rho = _gate_rows(a.conj().T.copy(), kind, t, qs, vs, off, mask, angle, data)
    return word_distribution(np.clip(np.real(np.diag(rho)), 0.0, None), meas_qubits, readout)


class NoisyNumpyEngine(NumpyEngine):
    """NumpyEngine with the noisy-shots entry point of qcmrf_amd._lib.Engine.  Numpy random numbers, not Philox: right
    in distribution only, never shot by shot (the per-shot reference is _philox_reference.exact_noisy_sample)"""

    calls = 0

    def noisy_sample(self, ops, data, shots, seed, meas_qubits=None, readout=None):
        if self.n_qubits > _lib.NOISY_MAX_QUBITS:
            raise ValueError("noisy shots: at most %d qubits" % _lib.NOISY_MAX_QUBITS)
        NoisyNumpyEngine.calls += 1
        rng = np.random.RandomState(seed % (2 ** 32))
        N, S = 1 << self.n_qubits, int(shots)
        psi = np.zeros((N, S), dtype=np.complex128)
        psi[0] = 1.0
        data = np.ascontiguousarray(data, dtype=np.float64)
        for kind, t, qs, vs, off, mask, angle in _records(ops, data):
            if kind in (_lib.OP_INIT_ZERO, _lib.OP_INIT_UNIFORM):
                psi[:] = _init_vector(N, kind, mask)[:, None]
            elif kind == _lib.OP_PAULI:
                cum = np.asarray(data[off:off + 4 ** len(qs)])
                draw = np.minimum(np.searchsorted(cum, rng.random_sample(S), side="right"), cum.size - 1)
                for p in np.unique(draw):
                    if p:
                        cols = np.flatnonzero(draw == p)
                        psi[:, cols] = _pauli_rows(psi[:, cols], qs, int(p))
            else:
                psi = _gate_rows(psi, kind, t, qs, vs, off, mask, angle, data)
        prob = np.abs(psi) ** 2
        cum = np.cumsum(prob, axis=0)
        r = rng.random_sample(S) * cum[-1]
        pick = np.minimum((cum <= r[None, :]).sum(axis=0), N - 1).astype(np.uint64)
        if meas_qubits is None:
            return pick
        out = np.zeros(S, dtype=np.uint64)
        for j, q in enumerate(meas_qubits):
            if q < 0:
                continue
            bit = (pick >> np.uint64(q)) & np.uint64(1)
            if readout is not None:
                f = np.asarray(readout, dtype=np.float64).reshape(-1, 2)[j][bit.astype(np.int64)]
                bit ^= (rng.random_sample(S) < f).astype(np.uint64)
            out |= bit << np.uint64(j)
        return out


def chi2_pvalue(counts, probs, shots, min_expected=5.0):
    """Pearson chi^2 of a counts dict ({bitstring: n}, bitstrings = words, bit 0 rightmost) against a distribution over
    words; cells expected below ``min_expected`` are pooled into one.  Counts outside the support: p = 0."""
    from scipy.stats import chi2
    obs = np.zeros(probs.size)
    for k, v in counts.items():
        obs[int(k.replace(" ", ""), 2)] += v
    exp = probs * shots
    if (obs[exp <= 0] > 0).any():
        return 0.0
    big = exp >= min_expected
    o = list(obs[big]) + ([obs[~big].sum()] if (~big).any() else [])
    e = list(exp[big]) + ([exp[~big].sum()] if (~big).any() else [])
    o, e = np.array(o), np.array(e)
    keep = e > 0
    o, e = o[keep], e[keep]
    stat = float(((o - e) ** 2 / e).sum())
    return float(chi2.sf(stat, max(1, o.size - 1)))
