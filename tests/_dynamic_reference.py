"""Numpy references for dynamic record streams (test infrastructure): ``_kraus2_reference`` extended by ``QSV_OP_IF`` and
``QSV_OP_RESET`` (include/qsv.h), without touching it.

  exact_dynamic_sample     exact per shot, by the documented contracts:
      IF (span, mask, value, negate): hit = ((word & mask) == value) != negate on the bits MEASURE records have written so far,
      as read (readout flip included; bits not yet written read 0); on a miss the next span records do nothing and take no draw
      -- the counter of stream 0 stands still, a skipped MEASURE writes no bit, and the ordinals of stream 3 are positions in
      the program.
      RESET on qubit t: the MEASURE rule with release = 1, u = u01(seed, shot, 3, d), d = the ordinal of the record among the
      MEASURE and RESET records; no classical bit, no readout draw.
      Every other kind as ``exact_kraus2_sample``.  Shots diverge, so every record runs on the columns that reach it.
  dynamic_distribution     exact as a distribution over the recorded words: one unnormalised rho per (word so far, records
      still to skip), branching on every written classical bit; no sampling.  For streams of a few written bits.
  DynamicNumpyEngine       the stand-in engine of the host tests (numpy random numbers: right in distribution only).

Written from the contract in include/qsv.h, not from the kernel.
"""
from __future__ import annotations

import numpy as np

from _density_matrix import _gate_rows, _init_vector, _pauli_channel, _pauli_probs, _records, word_distribution
from _kraus2_reference import Kraus2NumpyEngine, _apply_4x4, kraus2_of_record, kraus2_step
from _kraus_reference import _apply_2x2, check_kraus_words, kraus_of_record, kraus_step, within_cap  # noqa: F401 (re-exported)
from _measure_reference import (STREAM_MEASURE, MeasureNumpyEngine, _conj_apply, _rng_words, measure_of_record, measure_step)
from _philox_reference import STREAM_PAULI, STREAM_READOUT, STREAM_SAMPLE, TOL, pick_basis_state, record_words, u01
from _wide_reference import pauli_rows_wide
from qcmrf_amd import _lib

# ways a kernel could be wrong: the condition read before the readout flip; a skipped PAULI, KRAUS or KRAUS2 record still
# advancing the draw counter; the span off by one, either way; the whole word compared instead of the masked word; negate
# ignored; RESET projecting without moving the 1 half; RESET numbered among the MEASURE records only; RESET writing a bit
MUTATIONS = ("cond_before_flip", "skip_advances_draw", "span_plus_one", "span_minus_one", "whole_word", "ignore_negate",
             "reset_no_move", "reset_ordinal_measure_only", "reset_writes_bit")


def if_of_record(r):
    """(span, mask, value, negate) of an IF record"""
    lo, hi = int(r["vals"][0]) & 0xFFFFFFFF, int(r["vals"][1]) & 0xFFFFFFFF
    return int(r["n"]), int(r["mask"]), lo | (hi << 32), int(r["target"])


def _ordinals(rec, _mutate=None):
    """record index -> the draw number of stream 3: the ordinal among the MEASURE and RESET records, a position in the program"""
    out, n, n_measure = {}, 0, 0
    for i, r in enumerate(rec):
        k = int(r["kind"])
        if k in (_lib.OP_MEASURE, _lib.OP_RESET):
            out[i] = n_measure if _mutate == "reset_ordinal_measure_only" else n
            n += 1
            n_measure += k == _lib.OP_MEASURE
    return out


def exact_dynamic_sample(rec, data, W, shots, seed, meas_qubits=None, readout=None, first_shot=0, tol=TOL, block=1 << 21,
                         _mutate=None, _rng=None):
    """``_kraus2_reference.exact_kraus2_sample`` for programs that may hold IF and RESET records (module docstring).
    Returns (words, alt_words, ambiguous, undetermined), each of ``shots`` entries.  ``_rng`` (a numpy RandomState) replaces
    every Philox draw: the stand-in engine, right in distribution only."""
    if _mutate is not None and _mutate not in MUTATIONS:
        raise ValueError("unknown mutation %r" % (_mutate,))
    N, S = 1 << W, int(shots)
    seed = int(seed) & (2 ** 64 - 1)
    data = np.ascontiguousarray(data, dtype=np.float64)
    records = list(zip(rec, _records(rec, data)))
    ordinal = _ordinals(rec, _mutate)
    words = np.zeros(S, dtype=np.uint64)
    alt_words = np.zeros(S, dtype=np.uint64)
    ambiguous = np.zeros(S, dtype=bool)
    undetermined = np.zeros(S, dtype=bool)
    step = max(1, block // N)
    one = np.uint64(1)
    for lo in range(0, S, step):
        n = min(step, S - lo)
        shot = np.arange(lo, lo + n, dtype=np.uint64) + np.uint64(first_shot)

        def uni(stream, d, cols):
            if _rng is not None:
                return _rng.random_sample(n)[cols]
            return u01(seed, shot[cols], stream, d[cols] if isinstance(d, np.ndarray) else d)

        psi = np.zeros((N, n), dtype=np.complex128)
        psi[0] = 1.0
        draw = np.zeros(n, dtype=np.uint64)
        undet = np.zeros(n, dtype=bool)
        mword = np.zeros(n, dtype=np.uint64)
        raw = np.zeros(n, dtype=np.uint64)                  # the bits before their readout flip (mutation cond_before_flip only)
        resume = np.zeros(n, dtype=np.int64)                # a column runs record i iff i >= resume[column]
        for i, (r, (kind, t, qs, vs, off, mask, angle)) in enumerate(records):
            cols = np.flatnonzero(resume <= i)
            if _mutate == "skip_advances_draw" and kind in (_lib.OP_PAULI, _lib.OP_KRAUS, _lib.OP_KRAUS2):
                draw[resume > i] += one
            if cols.size == 0:
                continue
            full = cols.size == n                           # every column runs the record: no copy out and back
            sub = psi if full else psi[:, cols]
            if kind == _lib.OP_IF:
                span, cmask, value, negate = if_of_record(r)
                w = raw[cols] if _mutate == "cond_before_flip" else mword[cols]
                eq = (w == np.uint64(value)) if _mutate == "whole_word" else ((w & np.uint64(cmask)) == np.uint64(value))
                hit = eq if _mutate == "ignore_negate" else (eq != bool(negate))
                span += {"span_plus_one": 1, "span_minus_one": -1}.get(_mutate, 0)
                resume[cols[~hit]] = i + 1 + span
                continue
            if kind in (_lib.OP_INIT_ZERO, _lib.OP_INIT_UNIFORM):
                sub[:] = _init_vector(N, kind, mask)[:, None]
            elif kind == _lib.OP_PAULI:
                cum = data[off:off + 4 ** len(qs)]
                u = uni(STREAM_PAULI, draw, cols)
                p = np.minimum(np.searchsorted(cum, u, side="right"), cum.size - 1)    # first p with u < cum[p]
                draw[cols] += one
                for v in np.unique(p):
                    if v:
                        c2 = np.flatnonzero(p == v)
                        sub[:, c2] = pauli_rows_wide(sub[:, c2], qs, int(v))
            elif kind == _lib.OP_KRAUS:
                K, E = kraus_of_record(data, off, vs[0])
                u = uni(STREAM_PAULI, draw, cols)
                draw[cols] += one
                sub, _, ud = kraus_step(sub, qs[0], K, E, u, tol)
                undet[cols] |= ud
            elif kind == _lib.OP_KRAUS2:
                K, E = kraus2_of_record(data, off, vs[0])
                u = uni(STREAM_PAULI, draw, cols)
                draw[cols] += one
                sub, _, ud = kraus2_step(sub, qs[0], qs[1], K, E, u, tol)
                undet[cols] |= ud
            elif kind == _lib.OP_MEASURE:
                q, c, release, flips = measure_of_record(r, data)
                u = uni(STREAM_MEASURE, ordinal[i], cols)
                sub, b, ud = measure_step(sub, q, release, u, tol)
                undet[cols] |= ud
                bit = b ^ (uni(STREAM_READOUT, c, cols) < flips[b.astype(np.int64)]).astype(np.uint64)
                at = np.uint64(c)
                mword[cols] = (mword[cols] & ~(one << at)) | (bit << at)
                raw[cols] = (raw[cols] & ~(one << at)) | (b << at)
            elif kind == _lib.OP_RESET:
                u = uni(STREAM_MEASURE, ordinal[i], cols)
                sub, b, ud = measure_step(sub, qs[0], 0 if _mutate == "reset_no_move" else 1, u, tol)
                undet[cols] |= ud
                if _mutate == "reset_writes_bit":
                    mword[cols] = (mword[cols] & ~one) | b
            else:
                sub = _gate_rows(sub, kind, t, qs, vs, off, mask, angle, data)
            if full:
                psi = sub
            else:
                psi[:, cols] = sub
        every = np.arange(n)
        prob = psi.real * psi.real + psi.imag * psi.imag
        k, alt, amb = pick_basis_state(prob, uni(STREAM_SAMPLE, 0, every), tol)
        if _rng is not None:
            words[lo:lo + n] = _rng_words(k, meas_qubits, readout, _rng) | mword
            continue
        words[lo:lo + n] = record_words(k, seed, shot, meas_qubits, readout) | mword
        alt_words[lo:lo + n] = record_words(alt, seed, shot, meas_qubits, readout) | mword
        ambiguous[lo:lo + n] = amb
        undetermined[lo:lo + n] = undet
    return words, alt_words, ambiguous, undetermined


def dynamic_distribution(rec, data, n_qubits, meas_qubits, readout=None):
    """the exact distribution over the recorded words (2^len(meas_qubits) entries) of a program that may hold every record
    kind of ``qsv_noisy_sample``: an unnormalised rho per (word recorded so far, first record that runs again)"""
    N = 1 << n_qubits
    idx = np.arange(N)
    data = np.ascontiguousarray(data, dtype=np.float64)
    rho0 = np.zeros((N, N), dtype=np.complex128)
    rho0[0, 0] = 1.0
    branches = {(0, 0): rho0}

    def project(rho, q, b, move):
        m = ((idx >> q) & 1) == b
        part = rho * np.outer(m, m)
        if b == 1 and move:
            perm = idx ^ (1 << q)
            part = part[np.ix_(perm, perm)]
        return part

    for i, (r, (kind, t, qs, vs, off, mask, angle)) in enumerate(zip(rec, _records(rec, data))):
        new = {}

        def put(key, rho):
            new[key] = new[key] + rho if key in new else rho

        for (w, resume), rho in branches.items():
            if i < resume:
                put((w, resume), rho)
            elif kind == _lib.OP_IF:
                span, cmask, value, negate = if_of_record(r)
                hit = ((w & cmask) == value) != bool(negate)
                put((w, 0 if hit else i + 1 + span), rho)
            elif kind == _lib.OP_MEASURE:
                q, c, release, flips = measure_of_record(r, data)
                for b in (0, 1):
                    part = project(rho, q, b, release)
                    for flipped in (0, 1):
                        p = flips[b] if flipped else 1.0 - flips[b]
                        if p != 0.0:
                            put(((w & ~(1 << c)) | ((b ^ flipped) << c), 0), p * part)
            elif kind == _lib.OP_RESET:
                put((w, 0), project(rho, qs[0], 0, True) + project(rho, qs[0], 1, True))
            elif kind in (_lib.OP_INIT_ZERO, _lib.OP_INIT_UNIFORM):
                v = _init_vector(N, kind, mask)
                put((w, 0), np.outer(v, v.conj()) * np.trace(rho).real)
            elif kind == _lib.OP_PAULI:
                put((w, 0), _pauli_channel(rho, qs, _pauli_probs(data, off, len(qs))))
            elif kind == _lib.OP_KRAUS:
                K, _ = kraus_of_record(data, off, vs[0])
                put((w, 0), sum(_conj_apply(rho, lambda M, k=k: _apply_2x2(M, qs[0], k)) for k in K))
            elif kind == _lib.OP_KRAUS2:
                K, _ = kraus2_of_record(data, off, vs[0])
                put((w, 0), sum(_conj_apply(rho, lambda M, k=k: _apply_4x4(M, qs[0], qs[1], k)) for k in K))
            else:
                put((w, 0), _conj_apply(rho, lambda M: _gate_rows(M.copy(), kind, t, qs, vs, off, mask, angle, data)))
        branches = new
    dist = np.zeros(1 << len(meas_qubits))
    for (w, _), rho in branches.items():
        final = word_distribution(np.clip(np.real(np.diag(rho)), 0.0, None), meas_qubits, readout)
        np.add.at(dist, np.arange(final.size) | w, final)
    return dist


class DynamicNumpyEngine(Kraus2NumpyEngine):
    """Kraus2NumpyEngine whose noisy entry points also walk IF and RESET records.  Numpy random numbers: right in distribution
    only."""

    def _sample(self, limit, ops, data, shots, seed, meas_qubits, readout):
        if self.n_qubits > limit:
            raise ValueError("noisy shots: at most %d qubits" % limit)
        MeasureNumpyEngine.calls += 1
        rng = np.random.RandomState(seed % (2 ** 32))
        return exact_dynamic_sample(ops, data, self.n_qubits, shots, seed, meas_qubits, readout, _rng=rng)[0]
