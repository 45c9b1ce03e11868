"""Front end for circuits of the reference's construction (``QCMRF._build``, QCMRF.py:199-243): opening ``h`` gates and
extraction groups ``h a . B . x a . B' . x a . h a`` become the fused op list at once.

``compile_blocks(circuit)`` answers what ``ingest(circuit, peephole=True, compact=True)`` followed by
``passes.optimise(ops, level=3, fresh=True)`` answers -- the ``Ingested`` facts and ``[init] + diag factors`` -- or None.
The structure is matched in native code in one walk over ``circuit.data`` (``_ingest_native.read_circuit``, grammar in
DESIGN.md 4); the 128 ``ir.Op`` objects, the sets and the five passes over them that the pipeline spends on a 34-qubit
circuit are never built.  All floating-point arithmetic stays here, in the numpy calls the pipeline makes, on the same
operands in the same shapes, so the tables are the pipeline's bit for bit:

    ``M @ lam`` per block and one ``exp`` over all of them      ingest._finish_phase_blocks
    the batched sandwich product and ``ir.snap`` per table shape passes.fuse_sandwich
    column 0 of every 2x2 times sqrt 2, selects on |0> sliced    passes.fold_fresh, passes._slice_zero (here as indexing)

None means "not mine": the caller runs the pipeline, which decides or raises its own error.  Declining is always correct.

The run path (``QsvBackend._prepare``) takes the two halves apart: ``front_half`` is the walk, the facts and the floating-point
calls; then ``build_program`` does the fold's indexing, ``planner.plan`` and ``program.encode`` for the resulting init +
diagonal factors in one native call (``_ingest_native.build_program``: integers, comparisons with 0 and 1 and byte copies,
the same records and pool byte for byte), or, where that declines, ``fold_ops`` builds the op list here as before.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from . import ingest as _ingest
from . import ir
from . import planner
from . import program
from .passes import _SQRT2

_KEEP = {}


def _slice_zero(sel, mats, populated):
    """``passes._slice_zero`` on the (2^k, 2, 2) stack of a multiplexer, as indexing: the selects outside ``populated`` read
    |0>, so only the entries whose index has 0 there are kept.  Returns (surviving selects, their matrices); the index of a
    (number of selects, which of them survive) pattern is made once."""
    keep = 0
    for e, x in enumerate(sel):
        keep |= ((populated >> x) & 1) << e
    key = (len(sel), keep)
    idx = _KEEP.get(key)
    if idx is None:
        bits = [e for e in range(len(sel)) if (keep >> e) & 1]
        if bits == list(range(len(bits))):
            idx = slice(0, 1 << len(bits))                 # the survivors are the low index bits: a view
        else:
            j = np.arange(1 << len(bits))
            idx = np.zeros_like(j)
            for n, e in enumerate(bits):
                idx |= ((j >> n) & 1) << e
        if len(_KEEP) > 1024:
            _KEEP.clear()
        _KEEP[key] = idx
    return tuple([x for e, x in enumerate(sel) if (keep >> e) & 1]), mats[idx]


def _sandwich(t1, t2, u1, u2):
    """``passes.fuse_sandwich``'s product for one table shape: U2 diag(D2[s,1] D1[s,0], D2[s,0] D1[s,1]) U1 per select s"""
    ed = t2[:, :, ::-1] * t1                               # (batch, select, target value)
    return ir.snap(np.matmul(u2[:, None] * ed[:, :, None, :], u1[:, None]))


def _describe(circuit):
    """the native half: the compact description of ``circuit``, or None"""
    return _ingest._ingest_native.read_circuit(circuit)


def front_half(circuit, dense_kmax):
    """what both back halves start from: (Ingested facts, opened wires, groups, [(k, group indices, 2x2 stack)] per table
    shape), or None.  The native walk, the facts, and all floating-point arithmetic but the sqrt 2 of the fold."""
    if not _ingest.native_frontend_on():
        return None
    got = _describe(circuit)
    if got is None:
        return None
    nq, nc, opened, groups, measures, n_src = got
    if int(circuit.num_qubits) != nq or int(getattr(circuit, "num_clbits", 0)) != nc:
        return None
    # passes.fuse_dense looks at neighbouring ops that fit one window together; here it must find none
    for a, b in zip(groups, groups[1:]):
        if len(set(a[1]) | set(b[1])) <= dense_kmax:
            return None

    out = _ingest.Ingested(nq, nc)
    out.global_phase += float(getattr(circuit, "global_phase", 0.0) or 0.0)
    for c, q in measures:
        out.measure[c] = q
    out.n_source_ops = n_src
    cregs = getattr(circuit, "cregs", None)
    if cregs:
        out.creg_sizes = [(getattr(r, "name", "c"), len(r)) for r in cregs]
    out.ingest_path = "native"
    return out, opened, groups, _tables(groups)


def _tables(groups):
    """the floating-point half: [(k, indices of the groups on k qubits, their multiplexed 2x2s as one (n, 2^(k-1), 2, 2)
    stack)] in order of first occurrence"""
    # the tables of all blocks, B and B' of every group in program order: one exp (ingest._finish_phase_blocks)
    angs = []
    for _, _, blk1, lam1, blk2, lam2 in groups:
        angs.append(blk1[3] @ np.asarray(lam1, dtype=np.float64))
        angs.append(blk2[3] @ np.asarray(lam2, dtype=np.float64))
    tab = np.exp(1j * np.concatenate(angs))
    tables, off = [], 0
    for a in angs:
        tables.append(tab[off:off + a.size])
        off += a.size

    # one multiplexed 2x2 per group, all groups of one table shape in one product (passes.fuse_sandwich); the ancilla is
    # the last qubit of its blocks, so table-index bit k-1 is the target
    batches = {}
    for i, g in enumerate(groups):
        batches.setdefault(len(g[1]), []).append(i)
    h = ir.FIXED_1Q["h"]
    shapes = []
    for k, idx in batches.items():
        n = len(idx)
        t1 = np.moveaxis(np.stack([tables[2 * i] for i in idx]).reshape((n,) + (2,) * k), 1, -1).reshape(n, -1, 2)
        t2 = np.moveaxis(np.stack([tables[2 * i + 1] for i in idx]).reshape((n,) + (2,) * k), 1, -1).reshape(n, -1, 2)
        u = np.stack([h] * n)
        shapes.append((k, idx, _sandwich(t1, t2, u, u)))
    return shapes


def fold_ops(opened, groups, shapes):
    """[init] + the diagonal factors: every multiplexer acts on an ancilla still |0>, so it writes column 0 of its 2x2
    (passes.fold_fresh)"""
    mats = [None] * len(groups)
    for _, idx, m in shapes:
        for b, i in enumerate(idx):
            mats[i] = m[b]
    populated = 0
    for q in opened:
        populated |= 1 << q
    factors = []
    for g, m in zip(groups, mats):
        tg, sel = g[0], g[1][:-1]
        sq, st = _slice_zero(sel, m, populated)            # selects on qubits still |0> (the scratch wire always is)
        if not st[:, 1, 0].any() and np.array_equal(st, np.broadcast_to(np.eye(2), st.shape)):
            continue
        t = np.empty(2 * st.shape[0], dtype=np.complex128)
        np.multiply(st[:, :, 0].T, _SQRT2, out=t.reshape(2, -1))
        factors.append(ir.Op("diag", qubits=tuple(sq) + (tg,), table=t))
        populated |= 1 << tg
    return [ir.op_init(populated)] + factors


def compile_blocks(circuit, dense_kmax=5):
    """(Ingested, fused ops) of ``circuit`` as ingest + passes.optimise(level=3, fresh=True, dense_kmax=) give them, or
    None.  ``Ingested.ops`` stays empty: the ingested op list is never built (``QsvBackend.compile`` has it)."""
    front = front_half(circuit, dense_kmax)
    if front is None:
        return None
    return front[0], fold_ops(*front[1:])


def build_program(front, n_shards, layout):
    """(Plan, records, data pool) of what ``front_half`` answered, as ``planner.plan`` and ``program.encode`` give them for
    ``fold_ops``'s ops, or None: the fold's indexing, the layout and the records are made in one native call
    (``_ingest_native.build_program``).  Only the sqrt 2 of column 0 is multiplied here, once per table shape -- an
    element-wise product does not depend on how the array is cut.  None means "not mine", as everywhere in this module."""
    if not _ingest.native_program_on():
        return None
    ing, opened, groups, shapes = front
    got = _ingest._ingest_native.build_program(
        ing.num_qubits, opened, groups, [(k, m, np.multiply(m[..., 0], _SQRT2)) for k, _, m in shapes], n_shards, layout,
        ing.global_phase)
    if got is None:
        return None
    lay, rec, pool = got[:3]
    rec = np.frombuffer(rec, dtype=_lib.OP_DTYPE)
    data = np.frombuffer(pool, dtype=np.float64) if len(pool) else np.zeros(0, dtype=np.float64)
    pl = planner.Plan()
    pl.n_qubits, pl.n_shards = ing.num_qubits, n_shards
    pl.initial_layout, pl.layout = list(lay), list(lay)
    pl.ops = program.DecodedOps(rec, data)
    return pl, rec, data
