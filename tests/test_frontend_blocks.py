"""The native front end (qcmrf_amd/frontend.py, ``_ingest_native.read_circuit``) against the pipeline it stands in for:
``passes.optimise(ingest(qc, peephole=True, compact=True).ops, level=3, fresh=True, flat=...)``.  Equality is exact -- kinds,
qubit tuples, masks, table bytes, order, the Ingested facts, the encoded program -- and everything off the grammar is
declined, or answered as the pipeline answers it."""
import gc
import os
import subprocess
import sys

import numpy as np
import pytest

from qcmrf_amd import QCMRF, frontend, workloads
from qcmrf_amd import ingest as ing_mod
from qcmrf_amd.backend import QsvBackend
from qcmrf_amd.circuit import CircuitInstruction, Qubit

import _frontend_cases as fc

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(autouse=True)
def _switches_on():
    assert ing_mod.native_available(), "qcmrf_amd._ingest_native is not built (python -m qcmrf_amd.build)"
    assert ing_mod.use_native(True) is True and ing_mod.use_native_frontend(True) is True, "both switches are on by default"
    yield
    ing_mod.use_native(True)
    ing_mod.use_native_frontend(True)


@pytest.mark.parametrize("seed", fc.SEEDS)
@pytest.mark.parametrize("name", sorted(fc.ACCEPTED))
def test_accepted_and_equal_to_the_pipeline(name, seed):
    qc = fc.accepted(name, seed)
    ing, ops = fc.assert_accepted_and_equal(qc)
    assert ops[0].kind == "init" and all(o.kind == "diag" for o in ops[1:]) and ing.ops == []
    if name == "baseline4":
        assert qc.num_qubits == 34 and len(ops) == 20
    if name == "one_gamma_zero":
        d = [ci.operation.definition for ci in qc.data if ci.operation.name.startswith("cU_C")][0]
        assert len(d.data) == 9                               # three triples, not four
    if name == "barriers_no_measurements":
        assert ing.measure == {} and any(ci.operation.name == "barrier" for ci in qc.data)


@pytest.mark.parametrize("name", ["edge", "chain9", "config1", "barriers_no_measurements"])
def test_run_path_encodes_the_same_program(name):
    qc = fc.accepted(name)
    on, off = fc.program_bytes(qc, True), fc.program_bytes(qc, False)
    assert on[0] == "blocks" and off[0] == "passes"
    assert on[1:] == off[1:]


def test_global_phase_rides_as_in_the_pipeline():
    qc = fc.accepted("chain3")
    qc.global_phase = 0.3
    ing, ops = fc.assert_accepted_and_equal(qc)
    assert ing.global_phase == 0.3
    on, off = fc.program_bytes(qc, True), fc.program_bytes(qc, False)
    assert on[0] == "blocks" and on[1:] == off[1:]
    qc.global_phase = 0.0
    assert fc.program_bytes(qc, True)[1:] != on[1:]           # (the phase is in the program)


@pytest.mark.parametrize("spoil", fc.SPOILS)
def test_off_the_grammar_is_declined_or_equal(spoil):
    how = fc.declined_or_equal(fc.spoiled(spoil))
    if spoil == "gate_after_measure":
        assert how.startswith("ValueError") and "after it was measured" in how
    elif spoil == "wire_never_opened":
        assert how == "equal"                                 # an untouched control wire is in the grammar: its bit is sliced away
    else:
        assert how == "declined", how
    assert fc.declined_or_equal(fc.spoiled(None)) == "equal"  # the hand-built circuit itself is taken


def test_empty_definition_is_declined():
    c = [[0, 1], [1, 2]]
    th = fc.theta(c)
    th[:4] = [0.0] * 4                                        # every gamma of the first clique is 0: its cU_C is empty
    qc = QCMRF(c, th)
    assert len([ci for ci in qc.data if ci.operation.name == "cU_C0"][0].operation.definition.data) == 0
    assert fc.declined_or_equal(qc) == "declined"


def test_clique_of_eight_variables_is_declined():
    c = [list(range(8))]
    assert fc.declined_or_equal(QCMRF(c, fc.theta(c))) == "declined"
    c = [list(range(7))]
    assert fc.declined_or_equal(QCMRF(c, fc.theta(c))) == "equal"


def test_conditioned_instruction_is_left_to_the_pipeline():
    qc = fc.accepted("chain3")
    h0 = qc.data[0].operation
    h0.condition = (qc.clbits[0], 1)
    how = fc.declined_or_equal(qc)
    assert how.startswith("ValueError") and "classically conditioned" in how
    h0.condition = None
    assert fc.declined_or_equal(qc) == "equal"


def test_bits_that_are_not_the_circuits_objects():
    qc = fc.accepted("chain3")
    ci = qc.data[0]
    qc.data[0] = CircuitInstruction(ci.operation, [Qubit(None, 0)], ())
    how = fc.declined_or_equal(qc)
    assert how.startswith("ValueError") and "not in this circuit" in how
    qc = fc.accepted("chain3")
    k = next(i for i, ci in enumerate(qc.data) if ci.operation.name == "measure")
    ci = qc.data[k]
    qc.data[k] = CircuitInstruction(ci.operation, ci.qubits, [type(ci.clbits[0])(None, 0)])
    how = fc.declined_or_equal(qc)
    assert how.startswith("ValueError") and "not in this circuit" in how


def test_legacy_tuple_instructions_are_declined():
    qc = fc.accepted("chain3")
    qc.data = [(ci.operation, list(ci.qubits), list(ci.clbits)) for ci in qc.data]
    assert ing_mod._ingest_native.read_circuit(qc) is None
    assert fc.declined_or_equal(qc) == "declined"
    # ... and one level down, in a block: the reader leaves it to the Python code, so the front end does too
    qc = fc.accepted("chain3")
    d = [ci.operation.definition for ci in qc.data if ci.operation.name.startswith("cU_C")][0]
    d.data = [(ci.operation, list(ci.qubits), list(ci.clbits)) for ci in d.data]
    assert fc.declined_or_equal(qc) == "declined"


def test_neighbouring_groups_that_fit_one_dense_window_are_declined():
    """two one-vertex cliques: 2 variables + scratch + 2 ancillas = 5 qubits, where passes.fuse_dense opens a window"""
    c = [[0], [1]]
    assert fc.declined_or_equal(QCMRF(c, fc.theta(c))) == "declined"


def test_junk_is_declined_without_an_exception():
    for junk in (None, 3, "x", object(), [], {}):
        assert ing_mod._ingest_native.read_circuit(junk) is None


# ---- the comparison can fail: three mistakes planted in the Python half --------------------------------------------------

def _swap_blocks(real):
    def describe(circuit):
        got = real(circuit)
        if got is None:
            return None
        nq, nc, opened, groups, measures, n_src = got
        return nq, nc, opened, [(a, glob, b2, l2, b1, l1) for a, glob, b1, l1, b2, l2 in groups], measures, n_src
    return describe


def _no_flip(t1, t2, u1, u2):
    from qcmrf_amd import ir
    return ir.snap(np.matmul(u2[:, None] * (t2 * t1)[:, :, None, :], u1[:, None]))


def _keep_scratch(real):
    return lambda sel, mats, populated: real(sel, mats, populated | (1 << sel[-1]))


PLANTS = {"blocks_swapped": ("_describe", _swap_blocks), "x_flip_left_out": ("_sandwich", lambda real: _no_flip),
          "scratch_bit_kept": ("_slice_zero", _keep_scratch)}


@pytest.mark.parametrize("plant", sorted(PLANTS))
@pytest.mark.parametrize("name", sorted(fc.ACCEPTED))
def test_planted_mistakes_change_every_accepted_case(monkeypatch, name, plant):
    qc = fc.accepted(name)
    fc.assert_accepted_and_equal(qc)
    attr, make = PLANTS[plant]
    monkeypatch.setattr(frontend, attr, make(getattr(frontend, attr)))
    with pytest.raises(AssertionError):
        fc.assert_accepted_and_equal(qc)


# ---- switches, metadata, references ---------------------------------------------------------------------------------------

def test_switches():
    qc = fc.accepted("edge")
    assert frontend.compile_blocks(qc) is not None
    assert ing_mod.use_native_frontend(False) is True
    assert frontend.compile_blocks(qc) is None and fc.program_bytes(qc, False)[0] == "passes"
    assert ing_mod.use_native_frontend(True) is False
    assert ing_mod.use_native(False) is True                  # the front end is built on the reader: off with it
    assert frontend.compile_blocks(qc) is None
    be = QsvBackend()
    ing = be._prepare(qc, dict(be.options))[0]
    assert (ing.compile_path, ing.ingest_path) == ("passes", "python")
    ing_mod.use_native(True)
    ing = be._prepare(qc, dict(be.options))[0]
    assert (ing.compile_path, ing.ingest_path) == ("blocks", "native")


def test_other_options_take_the_pipeline():
    qc = fc.accepted("edge")
    be = QsvBackend()
    for change in ({"fusion": 2}, {"fold_fresh": False}, {"dynamic": True}):
        assert be._prepare(qc, dict(be.options, **change))[0].compile_path == "passes", change
    ing, pl = be.compile(qc)                                  # the public compile keeps the ingested op list
    assert ing.compile_path == "passes" and len(ing.ops) > 0


def test_allocated_blocks_do_not_grow():
    qc = fc.accepted("edge")
    bad = fc.spoiled("gate_between_blocks")
    d = qc.data[3].operation
    watched = [qc, bad, d, qc.qubits[0], qc.clbits[0], sys.intern("clbits"), sys.intern("operation")]
    read = ing_mod._ingest_native.read_circuit
    for _ in range(200):
        frontend.compile_blocks(qc)
        read(bad)
    gc.collect()
    refs = [sys.getrefcount(o) for o in watched]
    blocks = sys.getallocatedblocks()
    for _ in range(20000):
        got = read(qc)
        assert read(bad) is None
    assert got is not None
    del got
    for _ in range(500):
        out = frontend.compile_blocks(qc)
    del out
    gc.collect()
    grown = sys.getallocatedblocks() - blocks
    assert [sys.getrefcount(o) for o in watched] == refs
    assert grown < 200, grown
    got = read(qc)
    counts = [sys.getrefcount(got), sys.getrefcount(got[2]), sys.getrefcount(got[3]), sys.getrefcount(got[3][0]), sys.getrefcount(got[4])]
    assert counts == [2] * 5                                  # the answer is the caller's alone


def test_strict_qiskit_container_in_a_child_process():
    """the strict Qiskit double must be importable as ``qiskit`` before qcmrf_amd is: see tests/_frontend_worker.py"""
    env = dict(os.environ)
    env.pop("PYTHONPATH", None)
    r = subprocess.run([sys.executable, os.path.join(HERE, "_frontend_worker.py")], capture_output=True, text=True,
                       timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    assert "frontend strict worker ok" in r.stdout
