"""Exact per-shot reference of noisy shots at any width, and the wide cases of the slot path (test infrastructure).

``exact_wide_sample`` is ``_kraus_reference.exact_kraus_sample`` with one step replaced: the Pauli step of
``_density_matrix`` looks parities up in a table of 2^13 entries and so ends at 13 qubits; ``pauli_rows_wide`` takes the
parity of ``i & z`` from a popcount instead.  Everything else -- the record walk, the gates, the Kraus step, the final
draw, the recorded words, the Philox draws -- is the code the narrow references use, unchanged.

``_mutate`` makes the reference wrong on purpose, in the ways a kernel with wide records could be:
  q_trunc4        a listed qubit of a PAULI or DIAG record kept to 4 bits (``q & 15``)
  cmask_trunc16   a control mask kept to 16 bits: controls on qubits >= 16 are lost
  wave0_chunks    the final draw taken by one wave over chunks sized for four: only the first quarter of the state

``WIDE_CASES`` names every wide case test_gpu_noise_hbm.py runs; test_wide_reference.py walks the same dictionary on the host.
"""
from __future__ import annotations

import functools

import numpy as np

import _kraus_cases as kc
import _noise_exact_cases as nc
from _density_matrix import _gate_rows, _init_vector, _records, _tensor
from _kraus_reference import kraus_of_record, kraus_step
from _philox_reference import STREAM_PAULI, STREAM_SAMPLE, TOL, pick_basis_state, record_words, u01
from qcmrf_amd import _lib, program

MUTATIONS = ("q_trunc4", "cmask_trunc16", "wave0_chunks")


def parity(v):
    """popcount(v) & 1 of non-negative integers below 2^32"""
    v = np.asarray(v, dtype=np.int64).copy()
    for s in (16, 8, 4, 2, 1):
        v ^= v >> s
    return v & 1


def pauli_rows_wide(M, qubits, p):
    """rows of M (2-d) times the Pauli with index p on ``qubits``: new[i ^ x] = old[i] (-1)^|i & z| i^ny, any width"""
    x = z = ny = 0
    for j, q in enumerate(qubits):
        xb, zb = (p >> (2 * j)) & 1, (p >> (2 * j + 1)) & 1
        x |= xb << q
        z |= zb << q
        ny += xb & zb
    ph = (1j ** ny) * (1 - 2 * parity(np.arange(M.shape[0]) & z))
    A = M * ph[:, None]
    T, W = _tensor(A)
    axes = tuple(W - 1 - q for q in range(W) if (x >> q) & 1)
    return np.ascontiguousarray(np.flip(T, axis=axes) if axes else T).reshape(M.shape)


def _mutated(records, how):
    out = []
    for kind, t, qs, vs, off, mask, angle in records:
        if how == "q_trunc4" and kind in (_lib.OP_PAULI, _lib.OP_DIAG):
            qs = [q & 15 for q in qs]
        if how == "cmask_trunc16" and kind in (_lib.OP_1Q, _lib.OP_MCX, _lib.OP_MCPHASE):
            keep = [b for b, q in enumerate(qs) if q < 16]
            qs, vs = [qs[b] for b in keep], [vs[b] for b in keep]
        out.append((kind, t, qs, vs, off, mask, angle))
    return out


def exact_wide_sample(rec, data, W, shots, seed, meas_qubits=None, readout=None, first_shot=0, tol=TOL, block=1 << 21,
                      _mutate=None):
    """(words, alt_words, ambiguous, undetermined) of shots [first_shot, first_shot + shots): the contract of
    ``exact_kraus_sample``, for any W"""
    if _mutate is not None and _mutate not in MUTATIONS:
        raise ValueError("unknown mutation %r" % (_mutate,))
    N, S = 1 << W, int(shots)
    seed = int(seed) & (2 ** 64 - 1)
    data = np.ascontiguousarray(data, dtype=np.float64)
    records = _mutated(list(_records(rec, data)), _mutate)
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
                        psi[:, cols] = pauli_rows_wide(psi[:, cols], qs, int(v))
            elif kind == _lib.OP_KRAUS:
                K, E = kraus_of_record(data, off, vs[0])
                u = u01(seed, shot, STREAM_PAULI, draw)
                draw += np.uint64(1)
                psi, _, ud = kraus_step(psi, qs[0], K, E, u, tol)
                undet |= ud
            else:
                psi = _gate_rows(psi, kind, t, qs, vs, off, mask, angle, data)
        prob = psi.real * psi.real + psi.imag * psi.imag
        if _mutate == "wave0_chunks":
            prob[N // 4:] = 0.0
        k, alt, amb = pick_basis_state(prob, u01(seed, shot, STREAM_SAMPLE, 0), tol)
        words[lo:lo + n] = record_words(k, seed, shot, meas_qubits, readout)
        alt_words[lo:lo + n] = record_words(alt, seed, shot, meas_qubits, readout)
        ambiguous[lo:lo + n] = amb
        undetermined[lo:lo + n] = undet
    return words, alt_words, ambiguous, undetermined


# ---- the wide cases -------------------------------------------------------------------------------------------------------
# 14: the first size LDS cannot hold; 16: the last size whose qubits fit 4 bits; 17: the first qubit 16 and the first mask
# bit beyond 16.  Shots fall with the width so that a reference stays at two to three seconds of numpy (the Kraus step
# of the narrow reference, reused as it is, costs 0.2 s per record at 2^17 x 16): 48, 12 and 8 shots.
WIDE_SHOTS = {14: 48, 16: 12, 17: 8}
WIDE_INIT = {14: "uniform", 16: None, 17: "mid"}


def wide_ops(W):
    return kc.with_kraus(nc.random_ops(W, 9000 + W, n_random=8, init=WIDE_INIT[W]), W, np.random.RandomState(9500 + W))


def wide_case(W):
    rec, data = program.encode(wide_ops(W))
    return dict(W=W, rec=rec, data=data, shots=WIDE_SHOTS[W], seed=9900 + W, meas=None, readout=None)


def wide_meas_case():
    """W = 17 read into a permuted 20-bit register: qubit 16 on bit 0, unwritten bits, readout errors that include 0 and 1"""
    c = dict(wide_case(17))
    rng = np.random.RandomState(1717)
    meas = [16, 3, -1, 0, 15, 16, 9, -1] + [int(q) for q in rng.permutation(17)[:12]]
    ro = rng.uniform(0.0, 0.3, (len(meas), 2))
    ro[1] = (0.0, 1.0)
    ro[4] = (1.0, 0.0)
    ro[[j for j, q in enumerate(meas) if q < 0]] = 1.0             # a flip that must not happen
    c.update(meas=meas, readout=ro, seed=171717)
    return c


WIDE_CASES = {"W=%d" % W: functools.partial(wide_case, W) for W in sorted(WIDE_SHOTS)}
WIDE_CASES["W=17 permuted register"] = wide_meas_case


@functools.lru_cache(maxsize=None)
def case(name):
    return WIDE_CASES[name]()


def reference_of(c, **kw):
    return exact_wide_sample(c["rec"], c["data"], c["W"], c["shots"], c["seed"], c["meas"], c["readout"], **kw)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(words, alt_words, ambiguous, undetermined) of a named wide case: computed once, shared, left unchanged"""
    ref = reference_of(case(name))
    for a in ref:
        a.setflags(write=False)
    return ref
