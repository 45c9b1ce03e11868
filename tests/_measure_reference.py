"""Numpy references for noisy runs that measure in place (test infrastructure): ``_kraus_reference`` extended by
``QSV_OP_MEASURE`` (include/qsv.h), without touching it.

  exact_measure_sample           exact per shot, by the documented contract of a MEASURE record on qubit t, bit c:
      u = u01(seed, shot, 3, d), d = the ordinal of the record among the MEASURE records (the counter of stream 0 does
      not advance); r00, r11, total as for a Kraus record; b = 0 if r00 > 0 and r00 > u total, else 1 if r11 > 0, else 0;
      a state without mass stays as it is with b = 0; the other half of every pair zero, the kept half times
      sqrt(total / w_b); release and b = 1: the kept half moves to the 0 half; bit c of the word cleared, then set to b
      flipped iff u01(seed, shot, 2, c) < flip[b]; the final word = the word of the final draw | these bits.
      A shot is ``undetermined`` from the point where u total lies within TOL (the derived 1e-9 of ``_philox_reference``) of
      the total of r00 or of the total itself: the engine sums in its own order.
  measure_density_distribution   exact as a distribution: one unnormalised rho per recorded word, the classical bits
      carried along (branches that recorded the same word are added: nothing later depends on how a word came about).
  MeasureNumpyEngine             the stand-in engine of the host tests (numpy random numbers: right in distribution only).

Written from the contract in include/qsv.h, not from the kernel.  Any width: the Pauli step is ``_wide_reference``'s.
"""
from __future__ import annotations

import numpy as np

from _density_matrix import (_gate_rows, _init_vector, _pauli_channel, _pauli_probs, _records, _sl, _tensor,
                             word_distribution)
from _kraus_reference import KrausNumpyEngine, _apply_2x2, _pair_sums, check_kraus_words, kraus_of_record, kraus_step
from _philox_reference import STREAM_PAULI, STREAM_READOUT, STREAM_SAMPLE, TOL, pick_basis_state, record_words, u01
from _wide_reference import pauli_rows_wide
from qcmrf_amd import _lib

STREAM_MEASURE = 3

# ways a kernel could be wrong: the slot not returned to |0> on release, the draw not scaled by the state's total, the flip
# probability indexed by the wrong value, the bit written at the slot index instead of c, the draw taken from stream 0
# (and counted there)
MUTATIONS = ("no_release", "draw_not_scaled", "flip_wrong_value", "bit_at_slot", "draw_stream0")


def measure_of_record(r, data):
    """(qubit, classical bit, release, (P(flip | 0), P(flip | 1))) of a MEASURE record"""
    off = int(r["data_off"])
    return int(r["qubits"][0]), int(r["vals"][0]), int(r["vals"][1]), np.asarray(data[off:off + 2], dtype=np.float64)


def measure_step(psi, q, release, u, tol=TOL, _mutate=None):
    """one MEASURE record on the columns of psi with the uniforms u: (new psi, outcome b, undetermined)"""
    r00, r11, _ = _pair_sums(psi, q)
    total = r00 + r11
    r = u if _mutate == "draw_not_scaled" else u * total
    b = np.where((r00 > 0) & (r00 > r), 0, np.where(r11 > 0, 1, 0))
    w = np.where(b == 1, r11, r00)
    mass = w > 0
    undet = mass & ((np.abs(r - r00) <= tol * total) | (np.abs(r - total) <= tol * total))
    scale = np.sqrt(np.where(mass, total, 1.0) / np.where(mass, w, 1.0))
    out = psi.copy()
    T, W = _tensor(out)
    s0, s1 = _sl(W, {q: 0}), _sl(W, {q: 1})
    a0, a1 = T[s0].copy(), T[s1].copy()
    keep0, keep1 = mass & (b == 0), mass & (b == 1)
    move = keep1 if (release and _mutate != "no_release") else np.zeros_like(keep1)
    stay1 = keep1 & ~move
    T[s0] = np.where(keep0, a0 * scale, np.where(move, a1 * scale, np.where(mass, 0.0, a0)))
    T[s1] = np.where(stay1, a1 * scale, np.where(mass, 0.0, a1))
    return out, np.where(mass, b, 0).astype(np.uint64), undet


def exact_measure_sample(rec, data, W, shots, seed, meas_qubits=None, readout=None, first_shot=0, tol=TOL, block=1 << 21,
                         _mutate=None, _rng=None):
    """``exact_kraus_sample`` for programs that may hold MEASURE records (module docstring).
    Returns (words, alt_words, ambiguous, undetermined), each of ``shots`` entries.  ``_rng`` (a numpy RandomState) replaces
    every Philox draw: the stand-in engine, right in distribution only."""
    if _mutate is not None and _mutate not in MUTATIONS:
        raise ValueError("unknown mutation %r" % (_mutate,))
    N, S = 1 << W, int(shots)
    seed = int(seed) & (2 ** 64 - 1)
    data = np.ascontiguousarray(data, dtype=np.float64)
    records = list(zip(rec, _records(rec, data)))
    words = np.zeros(S, dtype=np.uint64)
    alt_words = np.zeros(S, dtype=np.uint64)
    ambiguous = np.zeros(S, dtype=bool)
    undetermined = np.zeros(S, dtype=bool)
    step = max(1, block // N)
    for lo in range(0, S, step):
        n = min(step, S - lo)
        shot = np.arange(lo, lo + n, dtype=np.uint64) + np.uint64(first_shot)

        def uni(stream, d):
            return _rng.random_sample(n) if _rng is not None else u01(seed, shot, stream, d)

        psi = np.zeros((N, n), dtype=np.complex128)
        psi[0] = 1.0
        draw = np.zeros(n, dtype=np.uint64)
        undet = np.zeros(n, dtype=bool)
        mword = np.zeros(n, dtype=np.uint64)
        ordinal = 0
        for r, (kind, t, qs, vs, off, mask, angle) in records:
            if kind in (_lib.OP_INIT_ZERO, _lib.OP_INIT_UNIFORM):
                psi[:] = _init_vector(N, kind, mask)[:, None]
            elif kind == _lib.OP_PAULI:
                cum = data[off:off + 4 ** len(qs)]
                u = uni(STREAM_PAULI, draw)
                p = np.minimum(np.searchsorted(cum, u, side="right"), cum.size - 1)    # first p with u < cum[p]
                draw += np.uint64(1)
                for v in np.unique(p):
                    if v:
                        cols = np.flatnonzero(p == v)
                        psi[:, cols] = pauli_rows_wide(psi[:, cols], qs, int(v))
            elif kind == _lib.OP_KRAUS:
                K, E = kraus_of_record(data, off, vs[0])
                u = uni(STREAM_PAULI, draw)
                draw += np.uint64(1)
                psi, _, ud = kraus_step(psi, qs[0], K, E, u, tol)
                undet |= ud
            elif kind == _lib.OP_MEASURE:
                q, c, release, flips = measure_of_record(r, data)
                if _mutate == "draw_stream0":
                    u = uni(STREAM_PAULI, draw)
                    draw += np.uint64(1)
                else:
                    u = uni(STREAM_MEASURE, ordinal)
                ordinal += 1
                psi, b, ud = measure_step(psi, q, release, u, tol, _mutate)
                undet |= ud
                value = (np.uint64(1) - b) if _mutate == "flip_wrong_value" else b
                bit = b ^ (uni(STREAM_READOUT, c) < flips[value.astype(np.int64)]).astype(np.uint64)
                at = np.uint64(q if _mutate == "bit_at_slot" else c)
                mword = (mword & ~(np.uint64(1) << at)) | (bit << at)
            else:
                psi = _gate_rows(psi, kind, t, qs, vs, off, mask, angle, data)
        prob = psi.real * psi.real + psi.imag * psi.imag
        k, alt, amb = pick_basis_state(prob, uni(STREAM_SAMPLE, 0), tol)
        if _rng is not None:
            words[lo:lo + n] = _rng_words(k, meas_qubits, readout, _rng) | mword
            continue
        words[lo:lo + n] = record_words(k, seed, shot, meas_qubits, readout) | mword
        alt_words[lo:lo + n] = record_words(alt, seed, shot, meas_qubits, readout) | mword
        ambiguous[lo:lo + n] = amb
        undetermined[lo:lo + n] = undet
    return words, alt_words, ambiguous, undetermined


def _rng_words(idx, meas_qubits, readout, rng):
    if meas_qubits is None:
        return idx.copy()
    out = np.zeros(idx.shape, dtype=np.uint64)
    for j, q in enumerate(meas_qubits):
        if q < 0:
            continue
        bit = (idx >> np.uint64(q)) & np.uint64(1)
        if readout is not None:
            f = np.asarray(readout, dtype=np.float64).reshape(-1, 2)[j][bit.astype(np.int64)]
            bit = bit ^ (rng.random_sample(idx.size) < f).astype(np.uint64)
        out |= bit << np.uint64(j)
    return out


def _conj_apply(rho, f):
    """A rho A^dg for a map f that applies A to the rows of a matrix"""
    return f(f(rho).conj().T.copy()).conj().T


def measure_density_distribution(rec, data, n_qubits, meas_qubits, readout=None):
    """the exact distribution over the recorded words (2^len(meas_qubits) entries) of a program that may hold MEASURE
    records: an unnormalised rho per word recorded so far"""
    N = 1 << n_qubits
    idx = np.arange(N)
    data = np.ascontiguousarray(data, dtype=np.float64)
    rho0 = np.zeros((N, N), dtype=np.complex128)
    rho0[0, 0] = 1.0
    branches = {0: rho0}
    for r, (kind, t, qs, vs, off, mask, angle) in zip(rec, _records(rec, data)):
        if kind == _lib.OP_MEASURE:
            q, c, release, flips = measure_of_record(r, data)
            new = {}
            for w, rho in branches.items():
                for b in (0, 1):
                    m = ((idx >> q) & 1) == b
                    part = rho * np.outer(m, m)
                    if b == 1 and release:
                        perm = idx ^ (1 << q)
                        part = part[np.ix_(perm, perm)]
                    for flipped in (0, 1):
                        p = flips[b] if flipped else 1.0 - flips[b]
                        if p == 0.0:
                            continue
                        w2 = (w & ~(1 << c)) | ((b ^ flipped) << c)
                        new[w2] = new.get(w2, 0.0) + p * part
            branches = new
            continue
        for w in list(branches):
            rho = branches[w]
            if kind in (_lib.OP_INIT_ZERO, _lib.OP_INIT_UNIFORM):
                v = _init_vector(N, kind, mask)
                rho = np.outer(v, v.conj()) * np.trace(rho).real
            elif kind == _lib.OP_PAULI:
                rho = _pauli_channel(rho, qs, _pauli_probs(data, off, len(qs)))
            elif kind == _lib.OP_KRAUS:
                K, _ = kraus_of_record(data, off, vs[0])
                rho = sum(_conj_apply(rho, lambda M, k=k: _apply_2x2(M, qs[0], k)) for k in K)
            else:
                rho = _conj_apply(rho, lambda M: _gate_rows(M.copy(), kind, t, qs, vs, off, mask, angle, data))
            branches[w] = rho
    dist = np.zeros(1 << len(meas_qubits))
    for w, rho in branches.items():
        final = word_distribution(np.clip(np.real(np.diag(rho)), 0.0, None), meas_qubits, readout)
        np.add.at(dist, np.arange(final.size) | w, final)
    return dist


def check_measure_words(got, words, alt_words, ambiguous, undetermined, family, label=""):
    """every word of a call with MEASURE records against ``exact_measure_sample``: ``check_kraus_words`` (equal where the
    reference is sure, undetermined and ambiguous shots within the one cap)"""
    check_kraus_words(got, words, alt_words, ambiguous, undetermined, family=family, label=label)


class MeasureNumpyEngine(KrausNumpyEngine):
    """KrausNumpyEngine whose noisy entry points also walk MEASURE records, with the width limits of the library.  Numpy
    random numbers: right in distribution only."""

    def _sample(self, limit, ops, data, shots, seed, meas_qubits, readout):
        if self.n_qubits > limit:
            raise ValueError("noisy shots: at most %d qubits" % limit)
        KrausNumpyEngine.calls += 1
        rng = np.random.RandomState(seed % (2 ** 32))
        return exact_measure_sample(ops, data, self.n_qubits, shots, seed, meas_qubits, readout, _rng=rng)[0]

    def noisy_sample(self, ops, data, shots, seed, meas_qubits=None, readout=None):
        return self._sample(_lib.NOISY_MAX_QUBITS, ops, data, shots, seed, meas_qubits, readout)

    def noisy_sample_hbm(self, ops, data, shots, seed, meas_qubits=None, readout=None):
        return self._sample(_lib.NOISY_HBM_MAX_QUBITS, ops, data, shots, seed, meas_qubits, readout)
