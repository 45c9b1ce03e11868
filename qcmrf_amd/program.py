"""Encode planned (physical) IR ops as the flat ``qsv_op`` records ``qsv_exec`` consumes
(include/qsv.h): one ctypes crossing per circuit instead of one per gate."""
from __future__ import annotations

import numpy as np

from . import _lib

_X = np.array([[0, 1], [1, 0]], dtype=np.complex128)


def encode(ops, n_meas=None):
    """list of ir.Op (physical qubits) -> (records: ndarray[OP_DTYPE], data: float64 pool).  n_meas: the classical bits of the
    call the records go to (needed by "if" ops, which read them: QSV_OP_IF, include/qsv.h)"""
    rec = np.zeros(len(ops), dtype=_lib.OP_DTYPE)
    pool = []
    top = 0
    kraus_seen = {}
    span_end, span_of = 0, -1                  # ops below span_end lie in the span of the 'if' op span_of

    def put(arr):
        nonlocal top
        flat = np.ascontiguousarray(arr, dtype=np.complex128).view(np.float64).ravel()
        pool.append(flat)
        off = top
        top += flat.size
        return off

    def put_real(arr):
        nonlocal top
        flat = np.ascontiguousarray(arr, dtype=np.float64).ravel()
        pool.append(flat)
        off = top
        top += flat.size
        return off

    def fill(r, qs, vals=None):
        n = len(qs)
        if n > _lib.MAX_CTRL:
            raise ValueError("gate touches %d qubits; the engine's limit per gate is %d" % (n, _lib.MAX_CTRL))
        r["n"] = n
        r["qubits"][:n] = qs
        if vals is not None:
            r["vals"][:n] = vals

    for i, (r, op) in enumerate(zip(rec, ops)):
        k = op.kind
        if op.new_pass:
            r["flags"] = _lib.OPF_NEW_PASS
        if k == "init":
            r["kind"] = _lib.OP_INIT_UNIFORM if op.mask else _lib.OP_INIT_ZERO
            r["mask"] = op.mask
        elif k == "u":
            r["kind"] = _lib.OP_1Q
            r["target"] = op.target
            fill(r, op.ctrls, op.vals)
            r["data_off"] = put(op.mat)
        elif k == "x":
            r["kind"] = _lib.OP_MCX
            r["target"] = op.target
            fill(r, op.ctrls, op.vals)
        elif k == "diag":
            r["kind"] = _lib.OP_DIAG
            fill(r, op.qubits)
            r["data_off"] = put(op.table)
        elif k == "mcphase":
            r["kind"] = _lib.OP_MCPHASE
            fill(r, op.qubits, op.vals)
            r["angle"] = op.angle
        elif k == "mux":
            if len(op.ctrls) > 10:
                raise ValueError("multiplexer with %d controls exceeds the engine limit of 10" % len(op.ctrls))
            r["kind"] = _lib.OP_MUX
            r["target"] = op.target
            fill(r, op.ctrls)
            r["data_off"] = put(op.mats)
        elif k == "kq":
            if len(op.qubits) > _lib.MAX_KQ:
                raise ValueError("dense gate on %d qubits exceeds the engine limit of %d" % (len(op.qubits), _lib.MAX_KQ))
            r["kind"] = _lib.OP_KQ
            fill(r, op.qubits)
            r["data_off"] = put(op.mat)
        elif k == "swap":
            r["kind"] = _lib.OP_SWAP
            fill(r, op.a, op.b)
        elif k == "pauli":
            r["kind"] = _lib.OP_PAULI
            fill(r, op.qubits)
            r["data_off"] = put_real(pauli_cumulative(op.table, len(op.qubits)))
        elif k == "kraus":
            ks = np.asarray(op.table, dtype=np.complex128)
            r["kind"] = _lib.OP_KRAUS
            fill(r, op.qubits, [len(ks)])
            flat = kraus_seen.get(id(op.table))                 # a model hands every gate the same stack
            if flat is None:
                flat = kraus_seen[id(op.table)] = kraus_tables(ks)
            r["data_off"] = put_real(flat)
        elif k == "kraus2":
            ks = np.asarray(op.table, dtype=np.complex128)
            if len(op.qubits) != 2 or op.qubits[0] == op.qubits[1]:
                raise ValueError("a kraus2 op acts on two distinct qubits, got %r" % (tuple(op.qubits),))
            r["kind"] = _lib.OP_KRAUS2
            fill(r, op.qubits, [len(ks)])
            flat = kraus_seen.get(id(op.table))                 # the E block once per distinct stack
            if flat is None:
                flat = kraus_seen[id(op.table)] = kraus2_tables(ks)
            r["data_off"] = put_real(flat)
        elif k == "measure":
            c, release = int(op.mask), int(bool(op.vals[0])) if len(op.vals) else 0
            if not 0 <= c < 64:
                raise ValueError("a measure op records into classical bit %d; noisy runs hold bits 0..63" % c)
            r["kind"] = _lib.OP_MEASURE
            fill(r, [op.target], [c])
            r["vals"][1] = release
            r["data_off"] = put_real(measure_flips(op.table))
        elif k == "reset":
            r["kind"] = _lib.OP_RESET
            fill(r, [op.target])
        elif k == "if":
            span, mask, negate = int(op.target), int(op.mask), int(op.vals[0]) if len(op.vals) else 0
            value = int(op.a[0]) if len(op.a) else 0
            if i < span_end:
                raise ValueError("op %d: an 'if' op inside the span of the 'if' op %d (guards do not nest)" % (i, span_of))
            if span < 1 or i + span > len(ops) - 1:
                raise ValueError("op %d: an 'if' op guards %d ops, %d follow it" % (i, span, len(ops) - 1 - i))
            if n_meas is None:
                raise ValueError("op %d: an 'if' op reads classical bits and needs the measurement map of the call (n_meas)" % i)
            if mask == 0:
                raise ValueError("op %d: an 'if' op compares no classical bit (mask 0)" % i)
            if mask < 0 or mask >> min(64, int(n_meas)):
                raise ValueError("op %d: an 'if' op reads classical bits %#x, outside the %d bits of the call" % (i, mask, min(64, int(n_meas))))
            if value & ~mask or value < 0:
                raise ValueError("op %d: the value %#x of an 'if' op has bits outside its mask %#x" % (i, value, mask))
            if negate not in (0, 1):
                raise ValueError("op %d: the negate flag of an 'if' op is 0 or 1, not %r" % (i, negate))
            span_end, span_of = i + 1 + span, i
            r["kind"] = _lib.OP_IF
            r["n"] = span
            r["target"] = negate
            r["mask"] = mask
            r["vals"][:2] = np.array([value & 0xFFFFFFFF, value >> 32], dtype=np.uint32).view(np.int32)
        else:
            raise ValueError("cannot encode op kind %r" % k)
        if k == "init" and i < span_end:
            raise ValueError("op %d: an 'init' op inside the span of the 'if' op %d" % (i, span_of))
    data = np.concatenate(pool) if pool else np.zeros(0, dtype=np.float64)
    return rec, data


class DecodedOps:
    """The op list of a program that was encoded without one (``frontend.build_program``): ``init`` and ``diag`` records and
    their pool read back into ``ir.Op`` on first access.  ``len()`` builds nothing: the run path asks for it on every run."""

    def __init__(self, rec, data):
        self._rec, self._data, self._ops = rec, data, None

    def _decoded(self):
        if self._ops is None:
            from . import ir
            ops = []
            for r in self._rec:
                kind = int(r["kind"])
                if kind in (_lib.OP_INIT_ZERO, _lib.OP_INIT_UNIFORM):
                    ops.append(ir.op_init(int(r["mask"])))
                elif kind == _lib.OP_DIAG:
                    n, off = int(r["n"]), int(r["data_off"])
                    ops.append(ir.Op("diag", qubits=tuple(int(q) for q in r["qubits"][:n]),
                                     table=self._data[off:off + (2 << n)].view(np.complex128).copy()))
                else:
                    raise ValueError("cannot decode op kind %d" % kind)
            self._ops = ops
        return self._ops

    def __len__(self):
        return len(self._rec)

    def __iter__(self):
        return iter(self._decoded())

    def __getitem__(self, i):
        return self._decoded()[i]

    def __repr__(self):
        return repr(self._decoded())


def pauli_cumulative(probs, n):
    """QSV_OP_PAULI data: the 4^n cumulative probabilities in Pauli index order (qcmrf_amd.noise), every entry
    from the last non-zero probability on exactly 1.0 -- a draw u in [0, 1) picks the first p with u < cum[p]"""
    p = np.asarray(probs, dtype=np.float64).ravel()
    if n < 1 or n > 2 or p.size != 4 ** n:
        raise ValueError("a Pauli op on %d qubit(s) needs 4^n = %d probabilities, got %d" % (n, 4 ** n, p.size))
    cum = np.cumsum(p)
    cum[int(np.flatnonzero(p > 0)[-1]):] = 1.0
    return cum


def measure_flips(flips):
    """QSV_OP_MEASURE data: (P(flip | 0), P(flip | 1)) of the measured (logical) qubit's readout error, zeros for none"""
    f = np.zeros(2) if flips is None else np.asarray(flips, dtype=np.float64).ravel()
    if f.size != 2 or not ((f >= 0.0) & (f <= 1.0)).all():
        raise ValueError("a measure op carries two flip probabilities in [0, 1], got %r" % (flips,))
    return f


def kraus_tables(ks):
    """QSV_OP_KRAUS data: the m operators (each row-major, re / im as for QSV_OP_1Q: 8 doubles), then for each
    E_k = K_k^dg K_k as (E00, E11, Re E01, Im E01): the branch weights of a shot are tr(E_k rho) of its own state"""
    ks = np.ascontiguousarray(ks, dtype=np.complex128)
    if ks.ndim != 3 or ks.shape[1:] != (2, 2) or not 1 <= len(ks) <= 4:
        raise ValueError("a Kraus op holds 1 to 4 operators of 2 x 2, got shape %s" % (ks.shape,))
    E = np.einsum("kai,kaj->kij", ks.conj(), ks)
    if np.abs(E.sum(axis=0) - np.eye(2)).max() > 1e-9:
        raise ValueError("the operators of a Kraus op do not sum to a channel (sum K^dg K != 1)")
    e = np.stack([E[:, 0, 0].real, E[:, 1, 1].real, E[:, 0, 1].real, E[:, 0, 1].imag], axis=1)
    return np.concatenate([ks.view(np.float64).ravel(), e.ravel()])


_K2_UPPER = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))


def kraus2_tables(ks):
    """QSV_OP_KRAUS2 data: the m operators (4 x 4, row-major, re / im: 32 doubles each, matrix index bit j on qubits[j]),
    then for each E_k = K_k^dg K_k 16 doubles: its 4 real diagonal entries, then its upper off-diagonal entries
    (0,1) (0,2) (0,3) (1,2) (1,3) (2,3) as (re, im)"""
    ks = np.ascontiguousarray(ks, dtype=np.complex128)
    if ks.ndim != 3 or ks.shape[1:] != (4, 4) or not 1 <= len(ks) <= 16:
        raise ValueError("a kraus2 op holds 1 to 16 operators of 4 x 4, got shape %s" % (ks.shape,))
    E = np.einsum("kai,kaj->kij", ks.conj(), ks)
    if np.abs(E.sum(axis=0) - np.eye(4)).max() > 1e-9:
        raise ValueError("the operators of a kraus2 op do not sum to a channel (sum K^dg K != 1)")
    e = np.empty((len(ks), 16))
    e[:, :4] = np.einsum("kii->ki", E).real
    for j, (a, b) in enumerate(_K2_UPPER):
        e[:, 4 + 2 * j] = E[:, a, b].real
        e[:, 5 + 2 * j] = E[:, a, b].imag
    return np.concatenate([ks.view(np.float64).ravel(), e.ravel()])


def run_stepwise(engine, ops):
    """Same program through the one-call-per-gate entry points (parity tests exercise both)."""
    for op in ops:
        k = op.kind
        if k == "init":
            engine.init_uniform(op.mask) if op.mask else engine.init_zero()
        elif k == "u":
            engine.apply_1q(op.target, op.mat, op.ctrls, op.vals)
        elif k == "x":
            engine.apply_mcx(op.ctrls, op.target, op.vals)
        elif k == "diag":
            engine.apply_diag(op.qubits, op.table)
        elif k == "mcphase":
            engine.apply_mcphase(op.qubits, op.angle, op.vals)
        elif k == "mux":
            engine.apply_mux(op.ctrls, op.target, op.mats)
        elif k == "kq":
            engine.apply_kq(op.qubits, op.mat)
        elif k == "swap":
            engine.swap_layout(op.a, op.b)
        else:
            raise ValueError("cannot run op kind %r" % k)
