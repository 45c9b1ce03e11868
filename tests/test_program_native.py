"""The native back half of the front end (``frontend.build_program``, ``_ingest_native.build_program``) against what it
stands in for: ``program.encode(QsvBackend._plan(ing, ops, n_shards, opts).ops)`` on the ops of ``frontend.compile_blocks``.
Equality is exact -- record bytes, pool bytes, both layouts, exchange and op counts, and the lazily decoded ops -- for every
accepted circuit, three theta seeds, 1 / 2 / 4 / 8 shards and both layout modes (local qubits below 14, from 14 to 32, and 33
or more).  Everything the Python code would treat differently is declined and then answered by the Python code.

The planted mistakes are planted in the REFERENCE (a register-bit tie broken the other way in ``planner.choose_layout``,
tables left in (select, target value) order, a populated bit that is not set): the native code has no switch that makes it
wrong, and a comparison that notices the mistake on one side notices it on the other."""
import builtins
import functools
import gc
import sys

import numpy as np
import pytest

from qcmrf_amd import _lib, frontend, ir, planner, program
from qcmrf_amd import ingest as ing_mod
from qcmrf_amd.backend import QsvBackend

import _frontend_cases as fc

SHARDS = (1, 2, 4, 8)
LAYOUTS = ("auto", "reference")
native = ing_mod._ingest_native.build_program if ing_mod.native_available() else None


@pytest.fixture(autouse=True)
def _switches_on():
    assert ing_mod.native_available(), "qcmrf_amd._ingest_native is not built (python -m qcmrf_amd.build)"
    assert ing_mod.use_native(True) is True and ing_mod.use_native_frontend(True) is True, "both switches are on by default"
    assert ing_mod.use_native_program(True) is True, "the switch is on by default"
    yield
    ing_mod.use_native(True)
    ing_mod.use_native_frontend(True)
    ing_mod.use_native_program(True)


@functools.lru_cache(maxsize=None)
def circuit(name, seed=fc.SEEDS[0]):
    return fc.accepted(name, seed)


def options(n_shards, layout):
    return dict(QsvBackend().options, layout=layout, devices=[0] * n_shards)


def reference(qc, n_shards, layout, untransposed=False):
    """(Plan, record bytes, pool bytes) of the Python path, or the text of its error"""
    got = frontend.compile_blocks(qc, dense_kmax=fc.dense_kmax_of(qc, n_shards))
    assert got is not None, "declined by the front end"
    ing, ops = got
    if untransposed:
        for op in ops[1:]:
            op.table = np.ascontiguousarray(op.table.reshape(2, -1).T).ravel()
    try:
        pl = QsvBackend._plan(ing, ops, n_shards, options(n_shards, layout))
    except ValueError as e:
        return str(e)
    rec, data = program.encode(pl.ops)
    return pl, np.asarray(rec).tobytes(), np.asarray(data).tobytes()


def built(qc, n_shards, layout):
    front = frontend.front_half(qc, fc.dense_kmax_of(qc, n_shards))
    assert front is not None, "declined by the front end"
    got = frontend.build_program(front, n_shards, layout)
    if got is None:
        return None
    pl, rec, data = got
    assert rec.dtype == _lib.OP_DTYPE and data.dtype == np.float64
    return pl, rec.tobytes(), data.tobytes()


def assert_same_program(got, ref):
    assert got is not None, "declined"
    (pa, ra, da), (pb, rb, db) = got, ref
    assert ra == rb, "records"
    assert da == db, "pool"
    assert pa.layout == pb.layout and pa.initial_layout == pb.initial_layout == pa.layout
    assert type(pa.layout) is list and all(type(p) is int for p in pa.layout)
    assert (pa.n_exchanges, pa.n_qubits, pa.n_shards) == (pb.n_exchanges, pb.n_qubits, pb.n_shards) and pa.n_exchanges == 0
    assert type(pa.ops) is program.DecodedOps and pa.ops._ops is None
    assert len(pa.ops) == len(pb.ops) and pa.ops._ops is None          # the run path asks for len() on every run: nothing is built
    fc.assert_ops_equal(list(pa.ops), pb.ops)
    assert pa.ops._ops is not None and pa.ops[0].kind == "init" and pa.ops[0] is pa.ops[0]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n_shards", SHARDS)
@pytest.mark.parametrize("seed", fc.SEEDS)
@pytest.mark.parametrize("name", sorted(fc.ACCEPTED))
def test_equal_to_plan_and_encode(name, seed, n_shards, layout):
    qc = circuit(name, seed)
    ref = reference(qc, n_shards, layout)
    got = built(qc, n_shards, layout)
    if isinstance(ref, str):                                  # more shard bits than qubits: the planner's own error
        assert qc.num_qubits <= n_shards.bit_length() - 1 and got is None
        with pytest.raises(ValueError) as e:
            be = QsvBackend()
            be._prepare(qc, options(n_shards, layout))
        assert str(e.value) == ref
        return
    assert_same_program(got, ref)
    L = qc.num_qubits - (n_shards.bit_length() - 1)
    if name == "baseline4":
        assert (L >= planner.GEN_TOP_MIN_L) == (n_shards <= 2) and len(got[0].ops) == 20
    if name in ("config1", "baseline2"):
        assert L < planner.GEN_TOP_MIN_L


def test_the_three_ranges_of_local_qubits_are_all_met():
    seen = set()
    for name in fc.ACCEPTED:
        for n_shards in SHARDS:
            L = circuit(name).num_qubits - (n_shards.bit_length() - 1)
            seen.add(0 if L < 1 else 1 if L < 14 else 2 if L < planner.GEN_TOP_MIN_L else 3)
    assert seen == {0, 1, 2, 3}


def test_run_path_takes_it_and_says_so():
    be = QsvBackend()
    for name in ("edge", "config1", "barriers_no_measurements"):
        qc = circuit(name)
        ing, pl, rec, data, n_shards, _ = be._prepare(qc, dict(be.options))
        assert (ing.compile_path, ing.plan_path, ing.ingest_path, n_shards) == ("blocks", "native", "native", 1)
        ref = reference(qc, 1, "auto")
        assert_same_program((pl, rec.tobytes(), data.tobytes()), ref)
        assert rec.flags.writeable and (data.flags.writeable or not data.size)


# ---- declined: the Python code answers, with its bytes or with its error ---------------------------------------------------

def _args(qc, n_shards=1, layout="auto", phase=0.0):
    ing, opened, groups, shapes = frontend.front_half(qc, fc.dense_kmax_of(qc, n_shards))
    return [ing.num_qubits, opened, groups, [(k, m, np.multiply(m[..., 0], np.sqrt(2.0))) for k, _, m in shapes], n_shards, layout, phase]


def _python_path(qc, opts):
    was = ing_mod.use_native_program(False)
    try:
        be = QsvBackend()
        ing, pl, rec, data, _, _ = be._prepare(qc, opts)
    finally:
        ing_mod.use_native_program(was)
    assert ing.plan_path == "python" and type(pl.ops) is list
    return ing.compile_path, rec.tobytes(), data.tobytes(), pl.layout


def test_direct_call_is_taken_and_every_departure_is_declined():
    qc = circuit("chain9")
    good = _args(qc)
    assert native(*good) is not None
    k, m, c0 = good[3][0]

    def changed(at, value):
        a = list(good)
        a[at] = value
        return a

    for bad in (changed(6, 0.3), changed(6, 0), changed(6, None), changed(5, "Auto"), changed(5, b"auto"), changed(5, None),
                changed(4, 3), changed(4, 0), changed(4, -2), changed(4, 2.0), changed(4, 1 << 18), changed(4, 1 << 70),
                changed(0, 17), changed(0, 0), changed(0, 65), changed(0, 18.0),
                changed(1, list(good[1])), changed(1, good[1] + (99,)), changed(1, good[1] + (-1,)), changed(1, good[1] + (1.0,)),
                changed(2, tuple(good[2])), changed(2, []), changed(2, good[2] + [good[2][0][:5]]), changed(2, good[2] + [None]),
                changed(3, []), changed(3, None), changed(3, [(k, m)]), changed(3, [(k + 1, m, c0)]), changed(3, [(k, m, c0), (k, m, c0)]),
                changed(3, [(k, m[:-1], c0)]), changed(3, [(k, m, c0[:-1])]), changed(3, [(k, m.astype(np.complex64), c0)]),
                changed(3, [(k, m.view(np.float64), c0)]), changed(3, [(k, m.reshape(len(m), -1, 4), c0)]),
                changed(3, [(k, np.asfortranarray(m), c0)]), changed(3, [(k, m, np.asfortranarray(c0))]),
                changed(3, [(k, np.concatenate([m, m])[::2], c0)]), changed(3, [(k, m.tolist(), c0)]), changed(3, [(k, m, None)]),
                good[:6], good + [None]):
        assert native(*bad) is None, bad[4:]
    assert native() is None and native(None) is None
    for groups in ([None], [()], [(0, None, None, None, None, None)], [(0, [0, 1], None, None, None, None)]):
        for shapes in ([], good[3]):
            assert native(good[0], good[1], groups, shapes, 1, "auto", 0.0) is None       # groups are looked at before any shape
    # a group whose target is not the last qubit of its blocks, a qubit twice in a group, a factor of more qubits than a record holds
    a, glob = good[2][0][0], good[2][0][1]
    assert native(*changed(2, [(glob[0],) + good[2][0][1:]] + good[2][1:])) is None
    assert native(*changed(2, [(a, (glob[0],) + glob[:-2] + (a,)) + good[2][0][2:]] + good[2][1:])) is None
    wide = tuple(range(_lib.MAX_CTRL + 1))
    big = np.zeros((1, 1 << _lib.MAX_CTRL, 2, 2), dtype=np.complex128)
    assert native(40, (0, 1), [(wide[-1], wide, None, None, None, None)], [(len(wide), big, np.ascontiguousarray(big[..., 0]))], 1, "auto", 0.0) is None
    assert native(*good) is not None


def test_a_global_phase_is_left_to_the_python_path():
    qc = fc.accepted("chain3")
    qc.global_phase = 0.3
    assert built(qc, 1, "auto") is None
    be = QsvBackend()
    ing, pl, rec, data, _, _ = be._prepare(qc, dict(be.options))
    assert (ing.compile_path, ing.plan_path) == ("blocks", "python")
    assert ("blocks", rec.tobytes(), data.tobytes(), pl.layout) == _python_path(qc, dict(be.options))
    plain = reference(circuit("chain3"), 1, "auto")
    assert rec.tobytes() == plain[1] and data.tobytes() != plain[2]    # the phase rides in the first table


@pytest.mark.parametrize("change,text", [({"layout": "best"}, "layout must be 'auto' or 'reference', not 'best'"),
                                         ({"devices": [0, 0, 0]}, "number of shards must be a power of two"),
                                         ({"devices": [0] * 16}, "4 qubits cannot be split into 16 shards")])
def test_declined_options_raise_the_python_paths_error(change, text):
    qc = circuit("edge")
    be = QsvBackend()
    opts = dict(be.options, **change)
    for on in (True, False):
        ing_mod.use_native_program(on)
        with pytest.raises(ValueError) as e:
            be._prepare(qc, opts)
        assert str(e.value) == text


def test_a_circuit_the_front_end_declines_is_planned_in_python():
    be = QsvBackend()
    ing, pl, _, _, _, _ = be._prepare(fc.spoiled("gate_between_blocks"), dict(be.options))
    assert (ing.compile_path, ing.plan_path) == ("passes", "python") and type(pl.ops) is list


def test_switches():
    qc = circuit("edge")
    be = QsvBackend()

    def paths():
        ing = be._prepare(qc, dict(be.options))[0]
        return ing.compile_path, ing.plan_path

    assert paths() == ("blocks", "native")
    assert ing_mod.use_native_program(False) is True and not ing_mod.native_program_on()
    assert paths() == ("blocks", "python")
    assert ing_mod.use_native_program(True) is False and ing_mod.native_program_on()
    assert ing_mod.use_native_frontend(False) is True and not ing_mod.native_program_on()
    assert paths() == ("passes", "python")
    ing_mod.use_native_frontend(True)
    assert ing_mod.use_native(False) is True and not ing_mod.native_program_on()      # built on the front end, which is built on the reader
    assert paths() == ("passes", "python")
    ing_mod.use_native(True)
    assert paths() == ("blocks", "native")
    for change in ({"fusion": 2}, {"fold_fresh": False}, {"dynamic": True}):
        assert be._prepare(qc, dict(be.options, **change))[0].plan_path == "python", change


# ---- the comparison can fail: three mistakes planted in the reference ------------------------------------------------------

def _tie_the_other_way(monkeypatch):
    """the first of the two register-bit sorts, key (uses, -q), with equal uses ordered by q instead"""
    def wrong(items, key=None, reverse=False):
        items = list(items)
        if key is not None and any(items) and all(type(key(q)) is tuple and len(key(q)) == 2 and key(q)[1] == -q for q in items):
            real = key
            key = lambda q: (real(q)[0], q)                   # noqa: E731
        return builtins.sorted(items, key=key, reverse=reverse)
    monkeypatch.setattr(planner, "sorted", wrong, raising=False)


def _stale_populated(monkeypatch):
    """the populated bit of the last target that was written is not set"""
    real = ir.op_init
    monkeypatch.setattr(frontend.ir, "op_init", lambda mask: real(mask & ~(1 << (mask.bit_length() - 1))))


def _register_rule_applies(qc, n_shards, layout):
    return layout == "auto" and qc.num_qubits - (n_shards.bit_length() - 1) >= 14


PLANTS = {"tie_the_other_way": (_tie_the_other_way, False, _register_rule_applies),
          "table_not_transposed": (lambda monkeypatch: None, True, lambda qc, n_shards, layout: True),
          "stale_populated_bit": (_stale_populated, False, lambda qc, n_shards, layout: True)}


@pytest.mark.parametrize("plant", sorted(PLANTS))
@pytest.mark.parametrize("name", sorted(fc.ACCEPTED))
def test_planted_mistakes_fail_every_case_they_touch(monkeypatch, name, plant):
    qc = circuit(name)
    set_up, untransposed, touches = PLANTS[plant]
    cases = [(s, lay) for s in SHARDS for lay in LAYOUTS if qc.num_qubits > s.bit_length() - 1]
    for n_shards, layout in cases:
        assert_same_program(built(qc, n_shards, layout), reference(qc, n_shards, layout))
    set_up(monkeypatch)
    touched = 0
    for n_shards, layout in cases:
        if touches(qc, n_shards, layout):
            touched += 1
            with pytest.raises(AssertionError):
                assert_same_program(built(qc, n_shards, layout), reference(qc, n_shards, layout, untransposed=untransposed))
        else:
            assert_same_program(built(qc, n_shards, layout), reference(qc, n_shards, layout, untransposed=untransposed))
    assert touched or plant == "tie_the_other_way" and qc.num_qubits < 14


# ---- references ---------------------------------------------------------------------------------------------------------

def test_allocated_blocks_do_not_grow():
    qc = circuit("chain9")
    good, bad = _args(qc, 2), _args(qc, 3)
    layout = good[5]
    watched = [good[1], good[2], good[2][0], good[3][0][1], good[3][0][2], layout, good[6], bad[3][0][1]]
    for _ in range(200):
        assert native(*good) is not None and native(*bad) is None
    gc.collect()
    refs = [sys.getrefcount(o) for o in watched]
    blocks = sys.getallocatedblocks()
    for _ in range(20000):
        got = native(*good)
        assert native(*bad) is None
    assert got is not None
    del got
    front = frontend.front_half(qc, 5)
    for _ in range(500):
        out = frontend.build_program(front, 2, "auto")
        len(out[0].ops), list(out[0].ops)
    del out, front
    gc.collect()
    grown = sys.getallocatedblocks() - blocks
    assert [sys.getrefcount(o) for o in watched] == refs
    assert grown < 200, grown
    got = native(*good)
    counts = [sys.getrefcount(got), sys.getrefcount(got[0]), sys.getrefcount(got[1]), sys.getrefcount(got[2])]
    assert counts == [2] * 4                                  # the answer is the caller's alone
    assert type(got[0]) is tuple and type(got[1]) is bytearray and type(got[2]) is bytearray
    ops = frontend.compile_blocks(qc, dense_kmax=fc.dense_kmax_of(qc, 2))[1]
    assert got[3] == ops[0].mask and got[4] == len(ops) == len(got[1]) // _lib.OP_DTYPE.itemsize      # populated (logical), number of ops
