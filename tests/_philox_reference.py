"""Philox-exact numpy reference of ``qsv_noisy_sample`` (test infrastructure): every output word of a call.

Every random number of a noisy call is a pure function of (seed, shot, stream, draw) through Philox-4x32-10
(include/qsv.h, qsv_noise.h), and every use of one is an exact comparison of doubles (``u < cum[p]``, ``u < flip``) that
a CPU computes identically.  So this reference predicts each word, not only the distribution of the words:

  philox4x32_10        the Random123 generator, vectorised
  u01                  the documented convention: counter = (draw, stream, shot lo, shot hi), key = (seed lo, seed hi),
                       u = ((c0 << 32 | c1) >> 11) * 2^-53; stream 0 = Pauli ops in program order, 1 = the final draw,
                       2 = the readout flip of bit j (draw = j)
  exact_noisy_sample   all shots evolved side by side (``_density_matrix``'s record walkers), one word per shot

The one freedom left is the final draw: the engine sums |amp|^2 in its own order with its own rounding, so a draw that
lands within rounding distance of a boundary of the cumulative mass may fall on either side.  Such shots are reported
as ``ambiguous`` together with the word of the neighbouring basis state.

Written from the documented convention and the Random123 definition of the round function, not from the kernel.
"""
from __future__ import annotations

import numpy as np

from _density_matrix import _gate_rows, _init_vector, _pauli_rows, _records
from qcmrf_amd import _lib

STREAM_PAULI, STREAM_SAMPLE, STREAM_READOUT = 0, 1, 2

# The engine promises amplitudes within 1e-12 of the numpy oracle for whole circuits (the bound every other kernel is
# held to).  An error of 1e-12 per amplitude moves a cumulative sum of |amp|^2 by at most 2 * 1e-12 * sum |amp| <=
# 2e-12 * 2^(W/2) of the total mass (Cauchy-Schwarz; 1.8e-10 at W = 13).  TOL = 1e-9 of the total mass is three decades
# above the per-amplitude promise and still covers that worst case; a draw lands that close to one of the at most 2^W
# boundaries with probability below 2 * 2^W * 1e-9 = 1.7e-5 per shot.  Derived, not tuned: it does not move.
TOL = 1e-9

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)          # Random123 philox4x32: multipliers
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)          # ... and Weyl key increments
_LO = np.uint64(0xFFFFFFFF)
_32 = np.uint64(32)


def philox4x32_10(counter4, key2):
    """Random123 philox4x32-10.  counter4: four and key2: two 32-bit words (ints or arrays, broadcast together);
    returns uint32[..., 4].  Per round: (hi0, lo0) = M0 * c0, (hi1, lo1) = M1 * c2,
    c <- (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0); the key is bumped by (W0, W1) before every round but the first."""
    words = [np.asarray(x, dtype=np.uint64) & _LO for x in list(counter4) + list(key2)]
    c0, c1, c2, c3, k0, k1 = [np.array(a) for a in np.broadcast_arrays(*words)]
    for r in range(10):
        if r:
            k0 = (k0 + _W0) & _LO
            k1 = (k1 + _W1) & _LO
        p0, p1 = _M0 * c0, _M1 * c2                              # 32 x 32 -> 64 bits: exact in uint64
        c0, c1, c2, c3 = (p1 >> _32) ^ c1 ^ k0, p1 & _LO, (p0 >> _32) ^ c3 ^ k1, p0 & _LO
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def words_to_u01(c0, c1):
    """((c0 << 32 | c1) >> 11) * 2^-53: the top 53 bits of the 64-bit word, so [0, 1) in steps of 2^-53"""
    v = ((np.asarray(c0, dtype=np.uint64) << _32) | np.asarray(c1, dtype=np.uint64)) >> np.uint64(11)
    return v.astype(np.float64) * 2.0 ** -53                    # v < 2^53: the conversion is exact


def u01(seed, shot, stream, draw):
    """the uniform double of (seed, shot, stream, draw); seed and shot are 64-bit, any argument may be an array"""
    seed = np.asarray(seed, dtype=np.uint64)
    shot = np.asarray(shot, dtype=np.uint64)
    out = philox4x32_10((draw, stream, shot & _LO, shot >> _32), (seed & _LO, seed >> _32))
    return words_to_u01(out[..., 0], out[..., 1])


def pick_basis_state(prob, u, tol=TOL):
    """prob: (N, S) |amp|^2 of S shots, u: (S,) uniforms.  Returns (k, alt, ambiguous):
    k    the first index with prob > 0 whose inclusive cumulative sum exceeds u * total; if none does (rounding), the
         last index with mass; 0 for a state without mass
    ambiguous, alt   u * total within tol * total of the inclusive cumulative boundary above k (alt = the next index
         with mass) or of the one below it (alt = the previous index with mass); alt = k elsewhere"""
    N, S = prob.shape
    cols = np.arange(S)
    cum = np.cumsum(prob, axis=0)
    total = cum[-1]
    r = u * total
    mass = prob > 0
    hit = mass & (cum > r[None, :])
    last = N - 1 - mass[::-1].argmax(axis=0)
    k = np.where(hit.any(axis=0), hit.argmax(axis=0), np.where(mass.any(axis=0), last, 0))
    rows = np.arange(N)[:, None]
    below = np.maximum.accumulate(np.where(mass, rows, -1), axis=0)            # last index with mass <= row
    above = np.minimum.accumulate(np.where(mass, rows, N)[::-1], axis=0)[::-1]  # first index with mass >= row
    prev = np.where(k > 0, below[np.maximum(k - 1, 0), cols], -1)
    nxt = np.where(k < N - 1, above[np.minimum(k + 1, N - 1), cols], N)
    upper = cum[k, cols]
    lower = np.where(prev >= 0, cum[np.maximum(prev, 0), cols], 0.0)
    near_up = (np.abs(r - upper) <= tol * total) & (nxt < N)
    near_lo = (np.abs(r - lower) <= tol * total) & (prev >= 0)
    alt = np.where(near_up, nxt, np.where(near_lo, prev, k))
    return k.astype(np.uint64), alt.astype(np.uint64), near_up | near_lo


def record_words(idx, seed, shot, meas_qubits, readout):
    """basis indices -> recorded words: bit j = qubit meas_qubits[j] (-1: stays 0; None: the full index), each measured
    bit flipped when u01(seed, shot, 2, j) < readout[j][value]"""
    if meas_qubits is None:
        return idx.copy()
    ro = None if readout is None else np.asarray(readout, dtype=np.float64).reshape(-1, 2)
    out = np.zeros(idx.shape, dtype=np.uint64)
    for j, q in enumerate(meas_qubits):
        if q < 0:
            continue
        bit = (idx >> np.uint64(q)) & np.uint64(1)
        if ro is not None:
            flip = u01(seed, shot, STREAM_READOUT, j) < ro[j][bit.astype(np.int64)]
            bit = bit ^ flip.astype(np.uint64)
        out |= bit << np.uint64(j)
    return out


def _swap_xz_of_qubit1(p):
    return (p & 3) | ((p >> 2) & 1) << 3 | ((p >> 3) & 1) << 2


MUTATIONS = ("swap_xz_q1", "no_draw_on_identity", "seed_lo_only")


def exact_noisy_sample(rec, data, W, shots, seed, meas_qubits=None, readout=None, first_shot=0, tol=TOL, block=1 << 21,
                       _mutate=None):
    """What ``qsv_noisy_sample`` returns for shots [first_shot, first_shot + shots) of a call, word by word.

    Returns (words, alt_words, ambiguous), each of ``shots`` entries.  Per shot: |0..0>; every record in program order
    (a Pauli record draws u = u01(seed, shot, 0, d), d counting the Pauli records met so far whatever they drew, and
    applies the first p with u < cum[p], capped at 4^n - 1); one basis state by ``pick_basis_state`` with
    u01(seed, shot, 1, 0); the word by ``record_words``.  ``ambiguous[s]``: the final draw of shot s lies within
    ``tol`` of the total mass of a boundary (see TOL above for where the figure comes from); ``alt_words[s]`` is then
    the word of the neighbouring basis state with mass, its readout flips recomputed for its own bit values, and
    equals ``words[s]`` elsewhere.

    ``_mutate`` (one of MUTATIONS) makes the reference wrong on purpose, the way a kernel could be: the tests of the
    comparison helper use it to show that the helper notices.  Shots are evolved ``block`` amplitudes at a time."""
    if _mutate is not None and _mutate not in MUTATIONS:
        raise ValueError("unknown mutation %r" % (_mutate,))
    N, S = 1 << W, int(shots)
    seed = int(seed) & (2 ** 64 - 1)
    if _mutate == "seed_lo_only":
        seed &= 0xFFFFFFFF
    data = np.ascontiguousarray(data, dtype=np.float64)
    records = list(_records(rec, data))
    words = np.zeros(S, dtype=np.uint64)
    alt_words = np.zeros(S, dtype=np.uint64)
    ambiguous = np.zeros(S, dtype=bool)
    step = max(1, block // N)
    for lo in range(0, S, step):
        n = min(step, S - lo)
        shot = np.arange(lo, lo + n, dtype=np.uint64) + np.uint64(first_shot)
        psi = np.zeros((N, n), dtype=np.complex128)
        psi[0] = 1.0
        draw = np.zeros(n, dtype=np.uint64)
        for kind, t, qs, vs, off, mask, angle in records:
            if kind in (_lib.OP_INIT_ZERO, _lib.OP_INIT_UNIFORM):
                psi[:] = _init_vector(N, kind, mask)[:, None]
            elif kind == _lib.OP_PAULI:
                cum = data[off:off + 4 ** len(qs)]
                u = u01(seed, shot, STREAM_PAULI, draw)
                p = np.minimum(np.searchsorted(cum, u, side="right"), cum.size - 1)    # first p with u < cum[p]
                draw += (p != 0).astype(np.uint64) if _mutate == "no_draw_on_identity" else np.uint64(1)
                for v in np.unique(p):
                    if v:
                        cols = np.flatnonzero(p == v)
                        pv = _swap_xz_of_qubit1(int(v)) if _mutate == "swap_xz_q1" and len(qs) == 2 else int(v)
                        psi[:, cols] = _pauli_rows(psi[:, cols], qs, pv)
            else:
                psi = _gate_rows(psi, kind, t, qs, vs, off, mask, angle, data)
        prob = psi.real * psi.real + psi.imag * psi.imag
        k, alt, amb = pick_basis_state(prob, u01(seed, shot, STREAM_SAMPLE, 0), tol)
        words[lo:lo + n] = record_words(k, seed, shot, meas_qubits, readout)
        alt_words[lo:lo + n] = record_words(alt, seed, shot, meas_qubits, readout)
        ambiguous[lo:lo + n] = amb
    return words, alt_words, ambiguous
