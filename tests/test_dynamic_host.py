"""Dynamic circuits on the host (no GPU): the circuit API, ingest(dynamic=True), the slot plan, the encoder's refusals, and
run(dynamic=True) on a stand-in engine that walks the record stream in numpy."""
import numpy as np
import pytest

import _dynamic_cases as dc
from _density_matrix import chi2_pvalue
from _dynamic_reference import DynamicNumpyEngine, dynamic_distribution
from qcmrf_amd import QCMRF, _lib, ingest as ing_mod, ir, program, trajectory
from qcmrf_amd.backend import QsvBackend
from qcmrf_amd.circuit import Clbit, IfElseOp, QuantumCircuit, Register
from qcmrf_amd.noise import NoiseModel


def backend(engine=DynamicNumpyEngine, **options):
    b = QsvBackend(**options)
    b._engine_factory = lambda n, devices=(0,), rank=None, world_size=None: engine(n, len(devices))
    return b


def kinds(ops):
    return [o.kind for o in ops]


# ---- the circuit API ---------------------------------------------------------------------------------------------------------

def test_circuit_api():
    qc = QuantumCircuit(3, 3)
    assert [ci.operation.name for ci in qc.reset([0, 2]).instructions] == ["reset", "reset"]
    got = qc.x(1).c_if(qc.clbits[2], 1)
    assert got.instructions[0].operation.condition == (qc.clbits[2], 1) and qc.data[-1].operation.condition == (qc.clbits[2], 1)
    qc.cx(0, 1).c_if(qc.cregs[0], 5)
    assert qc.data[-1].operation.condition == (qc.cregs[0], 5)
    qc.h([0, 1]).c_if(qc.clbits[0], 0)                      # reaches every instruction just added
    assert all(ci.operation.condition == (qc.clbits[0], 0) for ci in qc.data[-2:])
    with pytest.raises(TypeError):
        qc.x(0).c_if(3, 1)
    n = len(qc.data)
    with qc.if_test((qc.clbits[1], 1)):
        qc.x(0)
        qc.h(2)
    assert len(qc.data) == n + 1
    op = qc.data[-1].operation
    assert isinstance(op, IfElseOp) and op.name == "if_else" and op.condition == (qc.clbits[1], 1)
    assert [ci.operation.name for ci in op.blocks[0].data] == ["x", "h"] and op.blocks[1] is None
    with qc.if_test((qc.cregs[0], 2)) as else_:
        qc.x(0)
    with else_:
        qc.z(1)
    op = qc.data[-1].operation
    assert [ci.operation.name for ci in op.blocks[0].data] == ["x"] and [ci.operation.name for ci in op.blocks[1].data] == ["z"]
    assert len(qc.data) == n + 2 and list(qc.data[-1].qubits) == qc.qubits and list(qc.data[-1].clbits) == qc.clbits


# ---- ingest ------------------------------------------------------------------------------------------------------------------

def guards(ops):
    return [(i, o.target, o.mask, o.a[0], o.vals[0]) for i, o in enumerate(ops) if o.kind == "if"]


def test_ingest_active_reset():
    ing = ing_mod.ingest(dc.active_reset(), dynamic=True)
    assert kinds(ing.ops) == ["u", "measure", "if", "x", "measure"]
    assert guards(ing.ops) == [(2, 1, 1, 1, 0)] and (ing.n_if, ing.n_reset, ing.n_reuse) == (1, 0, 1) and ing.dynamic
    assert ing.measure == {0: 0, 1: 0}


def test_ingest_noise_of_a_conditioned_gate_lies_inside_its_span():
    ing = ing_mod.ingest(dc.active_reset(), noise=dc.x_error_model(), dynamic=True)
    assert kinds(ing.ops) == ["u", "measure", "if", "x", "pauli", "measure"] and guards(ing.ops) == [(2, 2, 1, 1, 0)]
    assert ing.n_pauli == 1


def test_ingest_shared_ancilla():
    qc, src = dc.shared_ancilla_qcmrf()
    ing = ing_mod.ingest(qc, dynamic=True)
    n = src.num_vertices
    assert ing.n_reset == len(dc.CHAIN3) and ing.n_if == 0 and ing.num_qubits == n + 2
    at = [i for i, o in enumerate(ing.ops) if o.kind == "reset"]
    assert all(ing.ops[i].target == n + 1 and ing.ops[i - 1].kind == "measure" and ing.ops[i - 1].target == n + 1 for i in at)


def test_ingest_register_condition():
    ing = ing_mod.ingest(dc.register_condition(), dynamic=True)
    (i, span, mask, value, negate), = guards(ing.ops)
    assert (span, mask, value, negate) == (1, 0b111, 5, 0) and ing.ops[i + 1].kind == "x" and ing.ops[i + 1].target == 3
    # a register that does not start at bit 0: the value is shifted to its position
    qc = QuantumCircuit(1, 5)
    hi = Register(2, "hi", Clbit)
    hi._bits = qc.clbits[3:5]
    qc.x(0).c_if(hi, 2)
    assert guards(ing_mod.ingest(qc, dynamic=True).ops) == [(0, 1, 0b11000, 0b10000, 0)]


def test_ingest_if_else():
    ing = ing_mod.ingest(dc.if_else_circuit(), dynamic=True)
    assert kinds(ing.ops) == ["u", "measure", "if", "x", "u", "if", "u", "measure"]
    assert guards(ing.ops) == [(2, 2, 1, 1, 0), (5, 1, 1, 1, 1)] and ing.n_if == 2


def test_ingest_composite_under_a_condition_is_one_span():
    inner = QuantumCircuit(2, name="pair")
    inner.h(0)
    inner.cx(0, 1)
    inner.x(1)
    qc = QuantumCircuit(2, 1)
    qc.measure(0, 0)
    qc.append(inner.to_instruction(), [0, 1]).operation.c_if(qc.clbits[0], 1)
    ing = ing_mod.ingest(qc, noise=dc.x_error_model(), dynamic=True)
    assert kinds(ing.ops) == ["measure", "if", "u", "x", "x", "pauli"] and guards(ing.ops) == [(1, 4, 1, 1, 0)]


def test_ingest_refusals():
    def conditioned(cond):
        qc = QuantumCircuit(2, 70)
        qc.x(0)
        qc.data[-1].operation.condition = cond
        return qc

    qc = QuantumCircuit(2, 2)
    with qc.if_test((qc.clbits[0], 1)):
        qc.x(0).c_if(qc.clbits[1], 1)
    with pytest.raises(ValueError, match="'x'.*nested"):
        ing_mod.ingest(qc, dynamic=True)
    qc = conditioned(None)
    qc.data[-1].operation.condition = (qc.clbits[64], 1)
    with pytest.raises(ValueError, match="'x' reads classical bit 64"):
        ing_mod.ingest(qc, dynamic=True)
    qc = conditioned(None)
    qc.data[-1].operation.condition = (qc.clbits[0], 2)
    with pytest.raises(ValueError, match="'x'.*does not fit"):
        ing_mod.ingest(qc, dynamic=True)
    three = Register(3, "r", Clbit)
    qc = conditioned(None)
    three._bits = qc.clbits[:3]
    qc.data[-1].operation.condition = (three, 8)
    with pytest.raises(ValueError, match="'x'.*does not fit"):
        ing_mod.ingest(qc, dynamic=True)
    for cond in ((None, 1), "c0 == 1", (three, 1.5)):
        with pytest.raises(ValueError, match="'x'"):
            ing_mod.ingest(conditioned(cond), dynamic=True)


def test_without_dynamic_the_old_messages_stand():
    qc = QuantumCircuit(1, 1)
    qc.reset(0)
    with pytest.raises(ValueError, match=r"^reset is not supported \(deferred-measurement engine\)$"):
        ing_mod.ingest(qc)
    with pytest.raises(ValueError, match=r"^classically conditioned operation 'x' is not supported$"):
        ing_mod.ingest(dc.active_reset())
    qc = QuantumCircuit(2, 2)
    qc.h(0); qc.measure(0, 0); qc.x(0)
    with pytest.raises(ValueError, match=r"^gate 'x' acts on qubit 0 after it was measured; mid-circuit measurement with later use of the "
                                         r"qubit is not supported$"):
        ing_mod.ingest(qc)
    for c in (dc.active_reset(), dc.reset_only_circuit()):
        with pytest.raises(ValueError, match="not supported"):
            backend().run(c, shots=10, seed_simulator=1)
        with pytest.raises(ValueError, match="not supported"):
            backend().run(c, shots=10, seed_simulator=1, noise_model=dc.readout_model())


# ---- the planner -------------------------------------------------------------------------------------------------------------

def test_plan_reused_qubit_keeps_its_slot():
    ing = ing_mod.ingest(dc.active_reset(), dynamic=True)
    items, width, finals = trajectory.plan_slots_dynamic(ing.ops)
    assert width == 1 and finals == [(0, 1)]
    assert [x for x in items if isinstance(x, tuple)] == [("measure", 0, 0, False, 0)]


def test_plan_measure_inside_a_span_releases_nothing():
    ops = [dc.ry(0, 1.0), dc.ry(1, 1.0), dc.measure(0, 0), dc.guard(1, 1, 1), dc.measure(1, 1), dc.ry(2, 0.5), dc.measure(2, 2)]
    items, width, finals = trajectory.plan_slots_dynamic(ops)
    inside = [x for x in items if isinstance(x, tuple) and x[0] == "measure" and x[2] == 1]
    assert inside == [("measure", 1, 1, False, 1)]
    assert width == 2 and finals == [(0, 2)]               # qubit 2 took the slot the first measure released, not the guarded one
    assert items[0].kind == "u" and [x.kind if not isinstance(x, tuple) else x[0] for x in items] == ["u", "u", "measure", "if", "measure", "u"]
    assert items[3].target == 1


def test_plan_trailing_reset_is_dropped_unless_its_slot_is_handed_on():
    ops = [dc.ry(0, 1.0), dc.cx(0, 1), dc.reset(0), dc.measure(1, 0)]
    items, width, finals = trajectory.plan_slots_dynamic(ops)
    assert width == 2 and finals == [(1, 0)] and not [x for x in items if isinstance(x, tuple)]
    ops = [dc.ry(0, 1.0), dc.cx(0, 1), dc.reset(0), dc.ry(2, 0.3), dc.measure(1, 0), dc.measure(2, 1)]
    items, width, finals = trajectory.plan_slots_dynamic(ops)      # qubit 2 moves into slot 0: it has to find |0> there
    assert width == 2 and [x for x in items if isinstance(x, tuple)] == [("reset", 0)] and finals == [(1, 0), (0, 1)]
    ops = [dc.ry(0, 1.0), dc.measure(0, 0), dc.guard(1, 1, 1), dc.reset(0)]            # guarded: it stays
    items, _, _ = trajectory.plan_slots_dynamic(ops)
    assert items[-1] == ("reset", 0)
    with pytest.raises(ValueError, match="nested"):
        trajectory.plan_slots_dynamic([dc.guard(2, 1, 1), dc.guard(1, 1, 1), dc.ry(0, 1.0)])


# ---- the encoder -------------------------------------------------------------------------------------------------------------

def test_encode_writes_the_two_kinds():
    rec, data = program.encode([dc.guard(2, (1 << 63) | 1, 1 << 63, 1), dc.reset(3), dc.ry(0, 0.1)], n_meas=64)
    assert rec["kind"].tolist() == [_lib.OP_IF, _lib.OP_RESET, _lib.OP_1Q]
    r = rec[0]
    assert (int(r["n"]), int(r["target"]), int(r["mask"])) == (2, 1, (1 << 63) | 1)
    assert ((int(r["vals"][0]) & 0xFFFFFFFF) | ((int(r["vals"][1]) & 0xFFFFFFFF) << 32)) == 1 << 63
    assert (int(rec[1]["n"]), int(rec[1]["qubits"][0])) == (1, 3)


@pytest.mark.parametrize("ops,n_meas,match", [
    ([dc.guard(0, 1, 1), dc.ry(0, 0.1)], 4, "guards 0 ops"),
    ([dc.guard(2, 1, 1), dc.ry(0, 0.1)], 4, "guards 2 ops, 1 follow"),
    ([dc.guard(1, 0, 0), dc.ry(0, 0.1)], 4, "compares no classical bit"),
    ([dc.guard(1, 1, 3), dc.ry(0, 0.1)], 4, "bits outside its mask"),
    ([dc.guard(1, 1 << 4, 0), dc.ry(0, 0.1)], 4, "outside the 4 bits of the call"),
    ([dc.guard(1, 1, 1), dc.ry(0, 0.1)], None, "needs the measurement map"),
    ([dc.guard(2, 1, 1), dc.guard(1, 1, 1), dc.ry(0, 0.1)], 4, "inside the span"),
    ([dc.guard(1, 1, 1), ir.Op("init", mask=0)], 4, "'init' op inside the span"),
    ([dc.guard(1, 1, 1, 2), dc.ry(0, 0.1)], 4, "negate flag"),
], ids=["span 0", "span past the end", "mask 0", "value outside mask", "mask past n_meas", "no map", "if in span", "init in span", "negate"])
def test_encode_refusals(ops, n_meas, match):
    with pytest.raises(ValueError, match=match):
        program.encode(ops, n_meas=n_meas)


# ---- run(dynamic=True) on the stand-in engine ----------------------------------------------------------------------------------

def counts_vector(counts, nbits):
    v = np.zeros(1 << nbits)
    for k, c in counts.items():
        v[int(k.replace(" ", ""), 2)] = c
    return v


@pytest.mark.parametrize("name", sorted(dc.CIRCUITS))
def test_run_dynamic_counts_follow_the_exact_distribution(name):
    qc, nm, shots = dc.CIRCUITS[name](), dc.readout_model(), 6000
    res = backend().run(qc, shots=shots, seed_simulator=77, noise_model=nm, dynamic=True).result()
    meta = res.metadata()
    assert meta["dynamic"] is True and meta["noisy_measure"] == "in_place" and meta["method"] == "noisy"
    ing, rec, data, clist, meas, readout, _, state, (mode, width, n_measure) = QsvBackend._prepare_noisy_dynamic(qc, nm, "lds")
    assert meta["n_if_ops"] == ing.n_if == int((rec["kind"] == _lib.OP_IF).sum())
    assert meta["n_reset_ops"] == int((rec["kind"] == _lib.OP_RESET).sum()) and meta["n_qubits"] == width
    p = dynamic_distribution(rec, data, width, meas, readout)
    got = counts_vector(res.get_counts(), len(meas))
    assert got.sum() == shots and not got[p == 0].any()
    pv = chi2_pvalue(res.get_counts(), p, shots)
    print(name, pv)
    assert pv > 1e-4


def test_run_dynamic_without_a_model_runs_the_ideal_circuit():
    res = backend().run(dc.active_reset(), shots=500, seed_simulator=3, dynamic=True).result()
    counts = res.get_counts()
    assert set(counts) <= {"00", "01"} and sum(counts.values()) == 500       # the second bit always reads 0
    assert res.metadata()["n_if_ops"] == 1 and res.metadata()["n_reset_ops"] == 0 and res.metadata()["noisy_state"] == "lds"


def test_static_circuit_runs_as_without_the_option():
    qc = QCMRF(dc.CHAIN3, dc.CHAIN3_THETA)
    nm = dc.readout_model()
    a = backend().run(qc, shots=300, seed_simulator=5, noise_model=nm).result()
    b = backend().run(qc, shots=300, seed_simulator=5, noise_model=nm, dynamic=True).result()
    assert a.get_counts() == b.get_counts() and "dynamic" not in b.metadata()
    assert a.metadata()["noisy_measure"] == b.metadata()["noisy_measure"] == "deferred"
    # and in a batch next to a dynamic one, under its own seed
    both = backend().run([dc.active_reset(), qc], shots=300, seed_simulator=4, noise_model=nm, dynamic=True).result()
    assert both.get_counts()[1] == a.get_counts() and both.results[0]["metadata"]["dynamic"] is True


def test_run_refusals():
    qc = dc.active_reset()
    with pytest.raises(ValueError, match="post_select"):
        backend().run(qc, shots=10, dynamic=True, post_select={0: 0})
    with pytest.raises(ValueError, match="method='trajectory'"):
        backend().run(qc, shots=10, dynamic=True, method="trajectory")
    with pytest.raises(ValueError, match="one device"):
        backend().run(qc, shots=10, dynamic=True, devices=(0, 0))

    class Two:
        rank, world = 0, 2

    with pytest.raises(ValueError, match="one process"):
        backend().run(qc, shots=10, dynamic=True, comm=Two())
    wide = QuantumCircuit(1, 65)
    wide.h(0); wide.measure(0, 0); wide.reset(0); wide.measure(0, 64)
    with pytest.raises(ValueError, match="at most 64 classical bits"):
        backend().run(wide, shots=10, dynamic=True)
    with pytest.raises(ValueError, match="noisy_state='hbm'"):
        big = QuantumCircuit(14, 1)
        big.h(range(14)); big.measure(0, 0); big.x(0).c_if(big.clbits[0], 1); big.cx(0, 1); big.measure(1, 0)
        backend().run(big, shots=10, dynamic=True)


def test_density_matrix_refuses_what_needs_branching():
    with pytest.raises(ValueError, match="classical conditions.*branching"):
        backend().run(dc.active_reset(), shots=10, dynamic=True, method="density_matrix")
    qc = QuantumCircuit(1, 2)
    qc.h(0); qc.measure(0, 0); qc.h(0); qc.measure(0, 1)
    with pytest.raises(ValueError, match="used again without a reset.*branching"):
        backend().run(qc, shots=10, dynamic=True, method="density_matrix")
    prepared, place = QsvBackend._prepare_density_dynamic(dc.reset_only_circuit(), NoiseModel(), None)
    rec = prepared[1]
    resets = rec[rec["kind"] == _lib.OP_MEASURE]
    assert place["n_reset"] == len(resets) == 2 and place["fix"] == (0, 0) and (resets["vals"][:, 1] == 1).all()
