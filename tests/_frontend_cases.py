"""TEST INFRASTRUCTURE: circuits for the native front end (qcmrf_amd/frontend.py) and the comparison with the pipeline it
stands in for.  Everything is built through the container's public methods (h, x, p, u, append, measure, barrier), so the
same cases run on the in-tree container and on the strict Qiskit double (tests/_frontend_worker.py)."""
import json
import os

import numpy as np

from qcmrf_amd import QCMRF, frontend, passes, planner, program, workloads
from qcmrf_amd import ingest as ing_mod
from qcmrf_amd.backend import QsvBackend
from qcmrf_amd.ingest import ingest
from qcmrf_amd.qcmrf import QuantumCircuit

HERE = os.path.dirname(os.path.abspath(__file__))
SEEDS = (1984, 7, 20261020)


def theta(cliques, seed=1984):
    return workloads.theta_halfnorm(workloads.dimension(cliques), seed=seed)


def _config1(seed):
    g = json.load(open(os.path.join(HERE, "golden", "config1.json")))
    return g["cliques"], g["theta"] if seed == SEEDS[0] else theta(g["cliques"], seed)


def _one_gamma_zero(seed):
    th = theta([[0, 1], [1, 2]], seed)
    th[2] = 0.0                                             # gamma = arccos(e^0) / 2 = 0: QCMRF skips that triple
    return [[0, 1], [1, 2]], th


# name -> (seed -> (cliques, theta, QCMRF keywords)): none of these may be declined
ACCEPTED = {
    "vertex": lambda s: ([[0]], theta([[0]], s), {}),                                   # W = 3
    "edge": lambda s: ([[0, 1]], theta([[0, 1]], s), {}),                               # W = 4
    "triangle": lambda s: ([[0, 1, 2]], theta([[0, 1, 2]], s), {}),                     # W = 5
    "chain3": lambda s: (workloads.chain(3), theta(workloads.chain(3), s), {}),
    "chain9": lambda s: (workloads.chain(9), theta(workloads.chain(9), s), {}),
    "config1": lambda s: _config1(s) + ({},),
    "baseline2": lambda s: (workloads.baseline_config(2)[1], theta(workloads.baseline_config(2)[1], s), {}),
    "baseline4": lambda s: (workloads.baseline_config(4)[1], theta(workloads.baseline_config(4)[1], s), {}),
    "clique7": lambda s: ([list(range(7))], theta([list(range(7))], s), {}),
    "barriers_no_measurements": lambda s: (workloads.chain(4), theta(workloads.chain(4), s),
                                           {"with_barriers": True, "with_measurements": False}),
    "one_gamma_zero": lambda s: _one_gamma_zero(s) + ({},),
}


def accepted(name, seed=SEEDS[0]):
    cliques, th, kw = ACCEPTED[name](seed)
    return QCMRF(cliques, th, **kw)


def assemble(cliques, th, spoil=None):
    """``QCMRF._build`` replayed by hand on a plain circuit, with one departure from the grammar (``spoil``)"""
    m = QCMRF(cliques, th)
    n, W = m.num_vertices, m.num_qubits
    qc = QuantumCircuit(W, W, name="hand")
    if spoil == "scratch_h":
        qc.h(n)
    for q in range(n):
        if spoil == "wire_never_opened" and q == 0:
            continue
        if spoil == "u_opens_a_wire" and q == 0:
            qc.u(np.pi / 2, 0.3, 0.1, q)
            continue
        qc.h(q)
    if spoil == "wire_opened_twice":
        qc.h(0)
    main = list(range(n + 1))
    first = 0
    for ii, C in enumerate(cliques):
        anc = n + 1 + ii
        cu = m._clique_unitary(ii, C, first)
        first += 2 ** len(C)
        if spoil == "ancilla_touched_before" and ii == 0:
            qc.p(0.2, anc)
        qc.h(anc)
        qc.append(cu, main + [anc])
        if spoil == "gate_between_blocks" and ii == 0:
            qc.p(0.3, anc)
        xw = 0 if (spoil == "x_on_another_wire" and ii == 0) else anc
        qc.x([xw])
        second = main + [anc]
        if spoil == "blocks_on_different_tuples" and ii == 0:
            second = [main[1], main[0]] + main[2:] + [anc]
        qc.append(cu.inverse(), second)
        qc.x([xw])
        qc.h(anc)
        if spoil == "ancilla_touched_after" and ii == 0:
            qc.p(0.2, anc)
        qc.measure(anc, anc)
        if spoil == "gate_after_measure" and ii == 0:
            qc.x(anc)
    qc.measure(range(n), range(n))
    return qc


# departures that the front end must decline, or answer exactly as the pipeline does (which may be an error of its own)
SPOILS = ("scratch_h", "wire_never_opened", "u_opens_a_wire", "wire_opened_twice", "ancilla_touched_before", "gate_between_blocks",
          "x_on_another_wire", "blocks_on_different_tuples", "ancilla_touched_after", "gate_after_measure")


def spoiled(spoil):
    c = workloads.chain(3)
    return assemble(c, theta(c), spoil)


def dense_kmax_of(qc, n_shards=1):
    return max(1, min(5, int(qc.num_qubits) - (max(1, n_shards).bit_length() - 1)))


def pipeline(qc, n_shards=1):
    """what the front end stands in for: (Ingested, fused ops)"""
    ing = ingest(qc, peephole=True, compact=True)
    return ing, passes.optimise(ing.ops, level=3, fresh=True, dense_kmax=dense_kmax_of(qc, n_shards), flat=ing.flat)


def assert_ops_equal(got, ref):
    assert [o.kind for o in got] == [o.kind for o in ref]
    for a, b in zip(got, ref):
        assert (a.qubits, a.mask, a.target, a.ctrls, a.vals) == (b.qubits, b.mask, b.target, b.ctrls, b.vals), (a, b)
        assert all(type(q) is int for q in a.qubits)
        assert (a.table is None) == (b.table is None) and a.mats is None and b.mats is None and a.mat is None and b.mat is None
        if a.table is not None:
            assert a.table.dtype == b.table.dtype and a.table.shape == b.table.shape
            assert np.array_equal(a.table, b.table) and a.table.tobytes() == b.table.tobytes()


def assert_facts_equal(a, b):
    assert (a.num_qubits, a.num_clbits, a.creg_sizes, a.n_source_ops) == (b.num_qubits, b.num_clbits, b.creg_sizes, b.n_source_ops)
    assert a.measure == b.measure and list(a.measure) == list(b.measure)
    assert a.global_phase == b.global_phase and type(a.global_phase) is type(b.global_phase)
    assert a.ingest_path == b.ingest_path == "native"
    assert (a.dynamic, a.flat, a.readout) == (b.dynamic, b.flat, b.readout)


def program_bytes(qc, front):
    """the record stream of the run path (``QsvBackend._prepare``: compile + plan + encode) with the front end on or off"""
    be = QsvBackend()
    was = ing_mod.use_native_frontend(front)
    try:
        ing, pl, rec, data, _, _ = be._prepare(qc, dict(be.options))
    finally:
        ing_mod.use_native_frontend(was)
    return ing.compile_path, bytes(np.asarray(rec).tobytes()), bytes(np.asarray(data).tobytes()), list(pl.layout)


def assert_accepted_and_equal(qc):
    got = frontend.compile_blocks(qc, dense_kmax=dense_kmax_of(qc))
    assert got is not None, "declined"
    ing, ops = pipeline(qc)
    assert_facts_equal(got[0], ing)
    assert_ops_equal(got[1], ops)
    eo_lane = True
    pa = planner.plan(got[1], got[0].num_qubits, 1, "auto", lane_targets=eo_lane, dyn_lanes=planner.DYN_LANES)
    pb = planner.plan(ops, ing.num_qubits, 1, "auto", lane_targets=eo_lane, dyn_lanes=planner.DYN_LANES)
    ra, rb = program.encode(pa.ops), program.encode(pb.ops)
    assert np.asarray(ra[0]).tobytes() == np.asarray(rb[0]).tobytes() and np.asarray(ra[1]).tobytes() == np.asarray(rb[1]).tobytes()
    return got


def declined_or_equal(qc):
    """"declined", "equal", or the pipeline's error text when it raises (then the front end must have declined)"""
    try:
        ing, ops = pipeline(qc)
    except Exception as e:                                   # the pipeline's own refusal: the front end leaves it to it
        assert frontend.compile_blocks(qc, dense_kmax=dense_kmax_of(qc)) is None
        return "%s: %s" % (type(e).__name__, e)
    got = frontend.compile_blocks(qc, dense_kmax=dense_kmax_of(qc))
    if got is None:
        return "declined"
    assert_facts_equal(got[0], ing)
    assert_ops_equal(got[1], ops)
    return "equal"
