"""Numpy references for noisy runs with two-qubit Kraus records (test infrastructure): ``_measure_reference`` (and through
it ``_kraus_reference``, ``_philox_reference`` and ``_density_matrix``) extended by ``QSV_OP_KRAUS2`` (include/qsv.h), without
touching any of them.

  kraus2_rho / kraus2_density_distribution   exact: rho -> sum_k K_k rho K_k^dg per KRAUS2 record
  exact_kraus2_sample                        exact per shot, by the documented contract of a KRAUS2 record on (t0, t1):
      u = u01(seed, shot, 0, d), d counting every PAULI, KRAUS and KRAUS2 record met so far (m = 1 included);
      a quad = the four amplitudes that differ in the bits t0 and t1 only, a_x with bit t0 = x & 1 and bit t1 = x >> 1;
      r[x][y] = sum a_x conj(a_y) over the quads, total = tr r; with the packed E_k of the record (4 real diagonal entries,
      then (0,1) (0,2) (0,3) (1,2) (1,3) (2,3) as re, im) w_k = sum_x E_xx r_xx + 2 sum_{x<y} (Re E_xy Re r_xy + Im E_xy Im r_xy);
      the first k with w_k > 0 whose inclusive cumulative sum (of the positive w) exceeds u total, else the last k with
      w_k > 0; every quad times K_k sqrt(total / w_k); a state without mass stays as it is.
  The engine sums r in its own order, so a draw with u total within TOL (1e-9, the derived tolerance of ``_philox_reference``)
  of the total of a cumulative boundary, the top one included, may fall on either side: such a shot is ``undetermined`` from
  there on and left out of the comparison; ``check_kraus_words`` counts those shots together with the final-draw ambiguous
  ones against ``ambiguity_cap``.
  Kraus2NumpyEngine                          the stand-in engine of the host tests (numpy random numbers: right in
                                             distribution only).

Written from the contract in include/qsv.h, not from the kernel.
"""
from __future__ import annotations

import numpy as np

from _density_matrix import _gate_rows, _init_vector, _pauli_channel, _pauli_probs, _records, _sl, _tensor, word_distribution
from _kraus_reference import _apply_2x2, check_kraus_words, kraus_of_record, kraus_step, within_cap  # noqa: F401 (re-exported)
from _measure_reference import (STREAM_MEASURE, MeasureNumpyEngine, _conj_apply, _rng_words, measure_of_record, measure_step)
from _philox_reference import STREAM_PAULI, STREAM_READOUT, STREAM_SAMPLE, TOL, pick_basis_state, record_words, u01
from _wide_reference import pauli_rows_wide
from qcmrf_amd import _lib

UPPER = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))

# ways a kernel could be wrong: the two qubits' bit significance swapped, the packed E entries read in another order (the
# off-diagonal block before the diagonal), an off-diagonal of r conjugated, no draw counted for a channel of one operator,
# the state's mass taken for 1 (no renormalisation, the draw not scaled by the total)
MUTATIONS = ("swap_bits", "e_wrong_order", "r_conj", "no_draw_on_m1", "no_renorm")


def kraus2_of_record(data, off, m):
    """(K: (m, 4, 4) complex, E: (m, 16) packed) of a KRAUS2 record"""
    K = np.ascontiguousarray(data[off:off + 32 * m]).view(np.complex128).reshape(m, 4, 4)
    E = np.asarray(data[off + 32 * m:off + 48 * m], dtype=np.float64).reshape(m, 16)
    return K, E


def _quad(M, q0, q1):
    """the four slices a_0..a_3 of the rows of M (views into a reshaped M), a_x with bit q0 = x & 1, bit q1 = x >> 1"""
    T, W = _tensor(M)
    return T, [_sl(W, {q0: x & 1, q1: x >> 1}) for x in range(4)]


def _apply_4x4(M, q0, q1, K):
    """rows of M (2-d) times the 4 x 4 matrix K on (q0, q1), matrix index bit j on q_j; returns a new array"""
    out = M.copy()
    T, sl = _quad(out, q0, q1)
    a = [T[s].copy() for s in sl]
    for x in range(4):
        T[sl[x]] = K[x, 0] * a[0] + K[x, 1] * a[1] + K[x, 2] * a[2] + K[x, 3] * a[3]
    return out


def _quad_sums(psi, q0, q1):
    """(rd: (4, S) real diagonal of r, ro: (6, S) complex r[x][y] for the UPPER pairs) for every column of psi"""
    T, sl = _quad(psi, q0, q1)
    a = [T[s].reshape(-1, psi.shape[1]) for s in sl]
    rd = np.stack([(v.real ** 2 + v.imag ** 2).sum(axis=0) for v in a])
    ro = np.stack([(a[x] * a[y].conj()).sum(axis=0) for x, y in UPPER])
    return rd, ro


def kraus2_step(psi, q0, q1, K, E, u, tol=TOL, _mutate=None):
    """one KRAUS2 record on the columns of psi with the uniforms u: (new psi, picked k, undetermined)"""
    if _mutate == "swap_bits":
        q0, q1 = q1, q0
    rd, ro = _quad_sums(psi, q0, q1)
    if _mutate == "r_conj":
        ro = ro.copy()
        ro[0] = ro[0].conj()                                          # r[0][1] alone: a kernel's slip in one term
    total = rd.sum(axis=0)
    r = u if _mutate == "no_renorm" else u * total
    Eu = np.concatenate([E[:, 4:], E[:, :4]], axis=1) if _mutate == "e_wrong_order" else E
    S = psi.shape[1]
    cum = np.zeros(S)
    pick = np.full(S, -1)
    last = np.full(S, -1)
    wpick = np.ones(S)
    wlast = np.ones(S)
    undet = np.zeros(S, dtype=bool)
    for k in range(len(K)):
        e = Eu[k]
        w = sum(e[x] * rd[x] for x in range(4))
        w = w + 2.0 * sum(e[4 + 2 * j] * ro[j].real + e[5 + 2 * j] * ro[j].imag for j in range(6))
        pos = w > 0
        cum = cum + np.where(pos, w, 0.0)
        undet |= pos & (np.abs(r - cum) <= tol * total)
        hit = pos & (pick < 0) & (cum > r)
        pick = np.where(hit, k, pick)
        wpick = np.where(hit, w, wpick)
        last = np.where(pos, k, last)
        wlast = np.where(pos, w, wlast)
    none = pick < 0
    pick = np.where(none, last, pick)
    wpick = np.where(none, wlast, wpick)
    out = psi.copy()
    for k in np.unique(pick):
        if k < 0:
            continue                                                # a state without mass stays as it is
        cols = np.flatnonzero(pick == k)
        scale = 1.0 if _mutate == "no_renorm" else np.sqrt(total[cols] / wpick[cols])
        out[:, cols] = _apply_4x4(psi[:, cols], q0, q1, K[k]) * scale
    return out, pick, undet


def exact_kraus2_sample(rec, data, W, shots, seed, meas_qubits=None, readout=None, first_shot=0, tol=TOL, block=1 << 21,
                        _mutate=None, _rng=None):
    """``_measure_reference.exact_measure_sample`` for programs that may hold KRAUS2 records (module docstring): every
    record kind of ``qsv_noisy_sample``.  Returns (words, alt_words, ambiguous, undetermined), each of ``shots`` entries.
    ``_rng`` (a numpy RandomState) replaces every Philox draw: the stand-in engine, right in distribution only."""
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
            elif kind == _lib.OP_KRAUS2:
                K, E = kraus2_of_record(data, off, vs[0])
                u = uni(STREAM_PAULI, draw)
                if not (_mutate == "no_draw_on_m1" and len(K) == 1):
                    draw += np.uint64(1)
                psi, _, ud = kraus2_step(psi, qs[0], qs[1], K, E, u, tol, _mutate)
                undet |= ud
            elif kind == _lib.OP_MEASURE:
                q, c, release, flips = measure_of_record(r, data)
                u = uni(STREAM_MEASURE, ordinal)
                ordinal += 1
                psi, b, ud = measure_step(psi, q, release, u, tol)
                undet |= ud
                bit = b ^ (uni(STREAM_READOUT, c) < flips[b.astype(np.int64)]).astype(np.uint64)
                mword = (mword & ~(np.uint64(1) << np.uint64(c))) | (bit << np.uint64(c))
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


def kraus2_rho(rec, data, W):
    """rho after the record stream from |0..0><0..0| (``_density_cases.numpy_rho`` with KRAUS2 records)"""
    N = 1 << W
    rho = np.zeros((N, N), dtype=np.complex128)
    rho[0, 0] = 1.0
    data = np.ascontiguousarray(data, dtype=np.float64)
    for kind, t, qs, vs, off, mask, angle in _records(rec, data):
        if kind in (_lib.OP_INIT_ZERO, _lib.OP_INIT_UNIFORM):
            v = _init_vector(N, kind, mask)
            rho = np.outer(v, v.conj())
        elif kind == _lib.OP_PAULI:
            rho = _pauli_channel(rho, qs, _pauli_probs(data, off, len(qs)))
        elif kind == _lib.OP_KRAUS:
            K, _ = kraus_of_record(data, off, vs[0])
            rho = sum(_conj_apply(rho, lambda M, k=k: _apply_2x2(M, qs[0], k)) for k in K)
        elif kind == _lib.OP_KRAUS2:
            K, _ = kraus2_of_record(data, off, vs[0])
            rho = sum(_conj_apply(rho, lambda M, k=k: _apply_4x4(M, qs[0], qs[1], k)) for k in K)
        else:
            rho = _conj_apply(rho, lambda M: _gate_rows(M.copy(), kind, t, qs, vs, off, mask, angle, data))
    return rho


def kraus2_density_distribution(rec, data, n_qubits, meas_qubits, readout=None):
    """the exact distribution over the recorded words of a program that may hold KRAUS2 records"""
    rho = kraus2_rho(rec, data, n_qubits)
    return word_distribution(np.clip(np.real(np.diag(rho)), 0.0, None), meas_qubits, readout)


class Kraus2NumpyEngine(MeasureNumpyEngine):
    """MeasureNumpyEngine whose noisy entry points also walk KRAUS2 records.  Numpy random numbers: right in distribution only."""

    def _sample(self, limit, ops, data, shots, seed, meas_qubits, readout):
        if self.n_qubits > limit:
            raise ValueError("noisy shots: at most %d qubits" % limit)
        MeasureNumpyEngine.calls += 1
        rng = np.random.RandomState(seed % (2 ** 32))
        return exact_kraus2_sample(ops, data, self.n_qubits, shots, seed, meas_qubits, readout, _rng=rng)[0]
