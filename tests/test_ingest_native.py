"""The native reader of clique-block signatures (qcmrf_amd/csrc/ingest_native.cpp) against the Python code it stands in
for: ``ingest`` with the switch on and off gives the same ``Ingested`` bit for bit, the reader's key is the Python key,
every shape off its fast path falls back and still matches, and it leaks no reference."""
import gc
import json
import os
import subprocess
import sys

import pytest

from qcmrf_amd import QCMRF, workloads
from qcmrf_amd import ingest as ing_mod
from qcmrf_amd.circuit import AND, Qubit, QuantumCircuit
from qcmrf_amd.ingest import ingest

from _ingest_compare import assert_keys_equal, assert_same, blocks_of, both, both_raise

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(autouse=True)
def _native_built():
    assert ing_mod.native_available(), "qcmrf_amd._ingest_native is not built (python -m qcmrf_amd.build)"
    assert ing_mod.use_native(True) is True, "the switch must be on by default where the module imports"
    yield
    ing_mod.use_native(True)


def _theta(cliques):
    return workloads.theta_halfnorm(workloads.dimension(cliques))


def _config1():
    g = json.load(open(os.path.join(HERE, "golden", "config1.json")))
    return g["cliques"], g["theta"]


CIRCUITS = {
    "clique2": lambda: ([[0, 1]], _theta([[0, 1]])),
    "clique3": lambda: ([[0, 1, 2]], _theta([[0, 1, 2]])),
    "config1": _config1,
    "chain4": lambda: (workloads.chain(4), _theta(workloads.chain(4))),
    "workload34": lambda: (workloads.baseline_config(4)[1], _theta(workloads.baseline_config(4)[1])),
}


@pytest.mark.parametrize("name", sorted(CIRCUITS))
def test_native_and_python_ingest_agree(name):
    cliques, theta = CIRCUITS[name]()
    qc = QCMRF(cliques, theta)
    n_blocks = assert_keys_equal(qc)
    assert n_blocks == 2 * len(cliques)
    if name == "clique3":
        d = blocks_of(qc)[0]
        assert len(d.data) == 24 and sum(ci.operation.name == "and" for ci in d.data) == 16
    if name == "workload34":
        assert qc.num_qubits == 34
    a, b = both(qc)
    assert a.ingest_path == "native" and b.ingest_path == "python"
    assert sum(o.kind == "diag" and len(o.qubits) > 1 for o in a.ops) == n_blocks
    assert_same(a, b)


def _clique3():
    return QCMRF([[0, 1, 2]], _theta([[0, 1, 2]]))


def _first_block(qc):
    return blocks_of(qc)[0]


def _falls_back(qc, expect_path="mixed"):
    """the native reader leaves the first block to the Python code, and the two settings of the switch agree"""
    assert ing_mod._ingest_native.read_block(_first_block(qc)) is None
    a, b = both(qc)
    assert a.ingest_path == expect_path, a.ingest_path
    assert_same(a, b)
    return a


def test_fallback_legacy_tuple_instructions():
    qc = _clique3()
    d = _first_block(qc)
    d.data = [(ci.operation, list(ci.qubits), list(ci.clbits)) for ci in d.data]
    a = _falls_back(qc)
    assert sum(o.kind == "diag" and len(o.qubits) > 1 for o in a.ops) == 2       # still recognised, by the Python reader
    # ... and one level down: an AND whose own definition holds tuples
    qc = _clique3()
    inner = _first_block(qc).data[0].operation.definition
    inner.data = [(ci.operation, list(ci.qubits), list(ci.clbits)) for ci in inner.data]
    _falls_back(qc)


def test_fallback_foreign_bits_raise_alike():
    """bits that are not the definition's own (the in-tree container's bits compare by identity: nothing is equal to them)"""
    qc = _clique3()
    d = _first_block(qc)
    ci = d.data[1]
    d.data[1] = type(ci)(ci.operation, [Qubit(None, 0), ci.qubits[1]], ())
    assert ing_mod._ingest_native.read_block(d) is None
    assert "not in this circuit" in both_raise(qc, ValueError)


def test_fallback_conditioned_cp():
    qc = _clique3()
    _first_block(qc).data[1].operation.condition = (object(), 1)
    assert ing_mod._ingest_native.read_block(_first_block(qc)) is None
    assert "classically conditioned" in both_raise(qc, ValueError)


def test_fallback_open_control_cp():
    qc = _clique3()
    _first_block(qc).data[1].operation.ctrl_state = 0
    a = _falls_back(qc, "native")                                               # the other block of the circuit is one still
    assert any(o.kind == "mcphase" and tuple(o.vals) == (0, 1) for o in a.ops)


def test_triples_on_two_wire_sets_are_no_block():
    blk = QuantumCircuit(5, name="cU_C0")
    for ctrl, lam in ((0, 0.25), (1, -0.5)):
        blk.append(AND(1, [1]), [ctrl, 3])
        blk.cp(lam, 3, 4)
        blk.append(AND(1, [1]), [ctrl, 3])
    qc = QuantumCircuit(5, 5, name="two_wire_sets")
    qc.h(range(5))
    qc.append(blk.to_instruction(), list(range(5)))
    qc.measure(list(range(5)), list(range(5)))
    # the reader reads it (reading decides nothing); the table lookup says it is no block, on both paths
    got = ing_mod._ingest_native.read_block(_first_block(qc))
    assert got is not None and got[0] == ing_mod._read_block(_first_block(qc))[0]
    assert ing_mod._block_of_key(got[0]) is None
    a, b = both(qc)
    assert a.ingest_path == "python" and not any(o.kind == "diag" and len(o.qubits) > 1 for o in a.ops)
    assert_same(a, b)


def test_fallback_definition_with_global_phase():
    qc = _clique3()
    _first_block(qc).global_phase = 0.375
    a = _falls_back(qc, "native")
    assert a.global_phase == 0.375
    # ... and on an AND's definition: it is not unwrapped past the phase
    qc = _clique3()
    _first_block(qc).data[0].operation.definition.global_phase = 0.125
    _falls_back(qc, "native")


def test_block_on_a_measured_qubit_raises_alike():
    cliques = [[0, 1, 2]]
    src = QCMRF(cliques, _theta(cliques))
    block = next(ci for ci in src.data if ci.operation.name.startswith("cU_C"))
    n = src.num_qubits
    qc = QuantumCircuit(n, n, name="measured_first")
    qc.h(range(n))
    where = [src.find_bit(q).index for q in block.qubits]
    qc.measure(where[0], where[0])
    qc.append(block.operation, where)
    assert ing_mod._ingest_native.read_block(block.operation.definition) is not None     # the reader knows no measurements
    assert "after it was measured" in both_raise(qc, ValueError)


def test_string_parameter_raises_alike():
    qc = _clique3()
    _first_block(qc).data[4].operation.params = ["a quarter turn"]
    assert ing_mod._ingest_native.read_block(_first_block(qc)) is None
    assert both_raise(qc, ValueError) == "could not convert string to float: 'a quarter turn'"
    # a parameter that float() takes is taken: the angle is the float, on both paths
    qc = _clique3()
    _first_block(qc).data[4].operation.params = ["0.25"]
    a, b = both(qc)
    assert a.ingest_path == "native"
    assert_same(a, b)


def test_count_not_a_multiple_of_three():
    qc = _clique3()
    d = _first_block(qc)
    d.data = d.data[:-1]
    _falls_back(qc, "native")


def test_the_comparison_can_fail(monkeypatch):
    """a reader that swaps two positions of ``pos`` is caught, by the key comparison and by the ingest comparison"""
    qc = QCMRF(*CIRCUITS["config1"]())
    real = ing_mod._ingest_native.read_block

    def swapped(definition):
        got = real(definition)
        if got is None:
            return None
        (names, lens, pos, and_keys), lams = got
        assert pos[0] != pos[1]
        return (names, lens, (pos[1], pos[0]) + pos[2:], and_keys), lams

    d = _first_block(qc)
    assert swapped(d)[0] != ing_mod._read_block(d)[0]
    monkeypatch.setattr(ing_mod, "_native_read", swapped)
    a = ingest(qc, peephole=True)
    monkeypatch.setattr(ing_mod, "_native_read", None)
    b = ingest(qc, peephole=True)
    with pytest.raises(AssertionError):
        assert_same(a, b)


def test_switch():
    qc = _clique3()
    assert ing_mod.use_native(False) is True
    assert ingest(qc, peephole=True).ingest_path == "python"
    assert ing_mod.use_native(True) is False
    assert ingest(qc, peephole=True).ingest_path == "native"
    assert ingest(qc, peephole=False).ingest_path == "python"          # nothing is read as a block without the peephole


def test_reader_holds_no_reference():
    qc = _clique3()
    d = _first_block(qc)
    one_and = d.data[0].operation
    qubit = d.qubits[0]
    names = [one_and.name, sys.intern("operation"), sys.intern("ctrl_state")]
    watched = [qc, d, one_and, qubit] + names
    for _ in range(200):                                              # memo tables, small-int and float free lists: warm
        ingest(qc, peephole=True)
    gc.collect()
    refs = [sys.getrefcount(o) for o in watched]
    blocks = sys.getallocatedblocks()
    for _ in range(20000):
        ing = ingest(qc, peephole=True)
    assert ing.ingest_path == "native"
    del ing
    gc.collect()
    grown = sys.getallocatedblocks() - blocks
    assert [sys.getrefcount(o) for o in watched] == refs
    assert grown < 200, grown
    # the answers it gives away are the caller's alone
    got = ing_mod._ingest_native.read_block(d)
    assert sys.getrefcount(got) == 2
    key, lams = got
    del got
    assert sys.getrefcount(key) == 2 and sys.getrefcount(lams) == 2
    # ... and a fallback leaves nothing behind either, error indicator included
    d.data[1].operation.params = [object()]
    refs = [sys.getrefcount(o) for o in watched]
    for _ in range(2000):
        assert ing_mod._ingest_native.read_block(d) is None
    assert [sys.getrefcount(o) for o in watched] == refs


def test_strict_qiskit_shapes_in_a_child_process():
    """the strict Qiskit double must be importable as ``qiskit`` before qcmrf_amd is: see tests/_ingest_native_worker.py"""
    env = dict(os.environ)
    env.pop("PYTHONPATH", None)
    r = subprocess.run([sys.executable, os.path.join(HERE, "_ingest_native_worker.py")], capture_output=True, text=True,
                       timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    assert "ingest-native strict worker ok" in r.stdout
