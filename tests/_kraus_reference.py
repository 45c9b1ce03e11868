"""Numpy references for noisy runs with Kraus records (test infrastructure): ``_density_matrix`` and
``_philox_reference`` extended by ``QSV_OP_KRAUS`` (include/qsv.h), without touching either.

  kraus_density_distribution   exact as a distribution: rho -> sum_k K_k rho K_k^dg per Kraus record
  KrausNumpyEngine             NoisyNumpyEngine whose ``noisy_sample`` knows Kraus records (numpy random numbers:
                               right in distribution only); the stand-in engine of the host tests
  exact_kraus_sample           exact per shot, by the documented contract of a Kraus record:
      u = u01(seed, shot, 0, d), d counting every Pauli and Kraus record met so far (m = 1 included);
      r00 = sum |a_i0|^2, r11 = sum |a_i1|^2, r10 = sum a_i1 conj(a_i0) over the pairs of the target, total = r00 + r11;
      w_k = E00_k r00 + E11_k r11 + 2 Re(E01_k r10) with the E tables of the record;
      the first k with w_k > 0 whose inclusive cumulative sum (of the positive w) exceeds u total, else the last k with
      w_k > 0; every pair times K_k sqrt(total / w_k).
  The engine sums r in its own order, so a draw with u total within TOL (1e-9, the derived tolerance of the final draw in
  ``_philox_reference``) of the total of a cumulative boundary, the top one included, may fall on either side: such a
  shot is ``undetermined`` from there on and is left out of the comparison; ``check_kraus_words`` counts those shots
  together with the final-draw ambiguous ones against ``ambiguity_cap``.

Written from the contract in include/qsv.h, not from the kernel.
"""
from __future__ import annotations

import numpy as np

from _density_matrix import (NoisyNumpyEngine, _gate_rows, _init_vector, _pauli_channel, _pauli_probs, _pauli_rows,
                             _records, _sl, _tensor, word_distribution)
from _noise_exact_cases import ambiguity_cap, check_words
from _philox_reference import STREAM_PAULI, STREAM_SAMPLE, TOL, pick_basis_state, record_words, u01
from qcmrf_amd import _lib

# ways a kernel could be wrong: the state's mass taken for 1 (no renormalisation, the draw not scaled by the total), the E
# tables read in the wrong order, no draw counted for a channel of one operator, r10 conjugated
MUTATIONS = ("no_renorm", "e_wrong_order", "no_draw_on_m1", "r10_conj")


def kraus_of_record(data, off, m):
    """(K: (m, 2, 2) complex, E: (m, 4) = E00, E11, Re E01, Im E01) of a Kraus record"""
    K = np.ascontiguousarray(data[off:off + 8 * m]).view(np.complex128).reshape(m, 2, 2)
    E = np.asarray(data[off + 8 * m:off + 12 * m], dtype=np.float64).reshape(m, 4)
    return K, E


def _apply_2x2(M, q, K):
    """rows of M (2-d) times the 2 x 2 matrix K on qubit q; returns a new array"""
    out = M.copy()
    T, W = _tensor(out)
    s0, s1 = _sl(W, {q: 0}), _sl(W, {q: 1})
    a0, a1 = T[s0].copy(), T[s1].copy()
    T[s0] = K[0, 0] * a0 + K[0, 1] * a1
    T[s1] = K[1, 0] * a0 + K[1, 1] * a1
    return out


def kraus_density_distribution(rec, data, n_qubits, meas_qubits, readout=None):
    """``_density_matrix.density_distribution`` for programs that may hold Kraus records"""
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
        elif kind == _lib.OP_KRAUS:
            K, _ = kraus_of_record(data, off, vs[0])
            new = np.zeros_like(rho)
            for k in K:
                a = _apply_2x2(rho, qs[0], k)                       # K rho
                new += _apply_2x2(a.conj().T.copy(), qs[0], k).conj().T          # (K (K rho)^dg)^dg = K rho K^dg
            rho = new
        else:
            a = _gate_rows(rho.copy(), kind, t, qs, vs, off, mask, angle, data)
            rho = _gate_rows(a.conj().T.copy(), kind, t, qs, vs, off, mask, angle, data)
    return word_distribution(np.clip(np.real(np.diag(rho)), 0.0, None), meas_qubits, readout)


def _pair_sums(psi, q):
    """(r00, r11, r10) of qubit q for every column of psi"""
    T, W = _tensor(psi)
    a0 = T[_sl(W, {q: 0})].reshape(-1, psi.shape[1])
    a1 = T[_sl(W, {q: 1})].reshape(-1, psi.shape[1])
    r00 = (a0.real ** 2 + a0.imag ** 2).sum(axis=0)
    r11 = (a1.real ** 2 + a1.imag ** 2).sum(axis=0)
    return r00, r11, (a1 * a0.conj()).sum(axis=0)


def kraus_step(psi, q, K, E, u, tol=TOL, _mutate=None):
    """one Kraus record on the columns of psi with the uniforms u: (new psi, picked k, undetermined)"""
    r00, r11, r10 = _pair_sums(psi, q)
    if _mutate == "r10_conj":
        r10 = r10.conj()
    total = r00 + r11
    # "no_renorm": a kernel that takes the state's mass for 1, so neither rescales nor scales the draw.  The missing
    # scale alone could never show: it is uniform and every comparison is against the state's own total
    r = u if _mutate == "no_renorm" else u * total
    S = psi.shape[1]
    cum = np.zeros(S)
    pick = np.full(S, -1)
    last = np.full(S, -1)
    wpick = np.ones(S)
    wlast = np.ones(S)
    undet = np.zeros(S, dtype=bool)
    Eu = E[::-1] if _mutate == "e_wrong_order" else E
    for k in range(len(K)):
        w = Eu[k, 0] * r00 + Eu[k, 1] * r11 + 2.0 * (Eu[k, 2] * r10.real - Eu[k, 3] * r10.imag)
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
        out[:, cols] = _apply_2x2(psi[:, cols], q, K[k]) * scale
    return out, pick, undet


def exact_kraus_sample(rec, data, W, shots, seed, meas_qubits=None, readout=None, first_shot=0, tol=TOL, block=1 << 21,
                       _mutate=None):
    """``_philox_reference.exact_noisy_sample`` for programs that may hold Kraus records (module docstring).
    Returns (words, alt_words, ambiguous, undetermined), each of ``shots`` entries."""
    if _mutate is not None and _mutate not in MUTATIONS:
        raise ValueError("unknown mutation %r" % (_mutate,))
    N, S = 1 << W, int(shots)
    seed = int(seed) & (2 ** 64 - 1)
    data = np.ascontiguousarray(data, dtype=np.float64)
    records = list(_records(rec, data))
    words = np.zeros(S, dtype=np.uint64)
    alt_words = np.zeros(S, dtype=np.uint64)
    ambiguous = np.zeros(S, dtype=bool)
    undetermined = np.zeros(S, dtype=bool)
    step = max(1, block // N)
    for lo in range(0, S, step):
        n = min(step, S - lo)
        shot = np.arange(lo, lo + n, dtype=np.uint64) + np.uint64(first_shot)
        psi = np.zeros((N, n), dtype=np.complex128)
        psi[0] = 1.0
        draw = np.zeros(n, dtype=np.uint64)
        undet = np.zeros(n, dtype=bool)
        for kind, t, qs, vs, off, mask, angle in records:
            if kind in (_lib.OP_INIT_ZERO, _lib.OP_INIT_UNIFORM):
                psi[:] = _init_vector(N, kind, mask)[:, None]
            elif kind == _lib.OP_PAULI:
                cum = data[off:off + 4 ** len(qs)]
                u = u01(seed, shot, STREAM_PAULI, draw)
                p = np.minimum(np.searchsorted(cum, u, side="right"), cum.size - 1)    # first p with u < cum[p]
                draw += np.uint64(1)
                for v in np.unique(p):
                    if v:
                        cols = np.flatnonzero(p == v)
                        psi[:, cols] = _pauli_rows(psi[:, cols], qs, int(v))
            elif kind == _lib.OP_KRAUS:
                K, E = kraus_of_record(data, off, vs[0])
                u = u01(seed, shot, STREAM_PAULI, draw)
                if not (_mutate == "no_draw_on_m1" and len(K) == 1):
                    draw += np.uint64(1)
                psi, _, ud = kraus_step(psi, qs[0], K, E, u, tol, _mutate)
                undet |= ud
            else:
                psi = _gate_rows(psi, kind, t, qs, vs, off, mask, angle, data)
        prob = psi.real * psi.real + psi.imag * psi.imag
        k, alt, amb = pick_basis_state(prob, u01(seed, shot, STREAM_SAMPLE, 0), tol)
        words[lo:lo + n] = record_words(k, seed, shot, meas_qubits, readout)
        alt_words[lo:lo + n] = record_words(alt, seed, shot, meas_qubits, readout)
        ambiguous[lo:lo + n] = amb
        undetermined[lo:lo + n] = undet
    return words, alt_words, ambiguous, undetermined


def within_cap(ambiguous, undetermined):
    """undetermined shots plus final-draw ambiguous shots of a case against the one cap of the word-by-word tests"""
    n = int((ambiguous | undetermined).sum())
    return n, ambiguity_cap(ambiguous.size)


def check_kraus_words(got, words, alt_words, ambiguous, undetermined, family, label=""):
    """``check_words`` on the shots whose Kraus draws are determined; undetermined + ambiguous shots within the cap"""
    got = np.asarray(got, dtype=np.uint64)
    assert got.shape == words.shape, "%s %s: %d words for %d shots" % (family, label, got.size, words.size)
    n, cap = within_cap(ambiguous, undetermined)
    print("KRAUS family=%s case=%s shots=%d undetermined=%d ambiguous=%d" % (family, label, got.size, int(undetermined.sum()),
                                                                           int(ambiguous.sum())))
    assert n <= cap, "%s %s: %d undetermined or ambiguous shots of %d (cap %d)" % (family, label, n, got.size, cap)
    keep = ~undetermined
    check_words(got[keep], words[keep], alt_words[keep], ambiguous[keep], family=family, label=label)


class KrausNumpyEngine(NoisyNumpyEngine):
    """NoisyNumpyEngine that also walks Kraus records: per shot one operator drawn with its weight, applied, renormalised.
    Numpy random numbers: right in distribution only."""

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
            elif kind == _lib.OP_KRAUS:
                K, E = kraus_of_record(data, off, vs[0])
                psi, _, _ = kraus_step(psi, qs[0], K, E, rng.random_sample(S))
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
