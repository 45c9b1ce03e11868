"""qsv_sample_unordered / qsv_sample_cond_unordered against the ordered calls, and the native counts formatter through
QsvBackend.run.

Engine level: for one handle state, shots, seed and measurement map the sorted words of the unordered call equal the sorted
words of the ordered one, ``state_info`` moves as it does for the ordered call, and the errors keep their type and text.
Paths: the chain on a deferred shard (W = 14 and 16 at R = 4, one case at R = 6), a stored state, two virtual shards (the
host walk), sample_chain = 0, the post-selected call with a block bit and with an inner bit fixed.

Through run(): ``get_counts()`` is the same dict, insertion order included, with ``use_native_counts`` on and off, and
``counts_path`` in the metadata says which one ran.

Programs as in tests/test_gpu_sample_chain.py, from tests/_deferred_cases.py and tests/_factored_sum_model.py."""
import json
import os

import numpy as np
import pytest

import _deferred_cases as dc
import _factored_sum_model as fm

pytestmark = pytest.mark.gpu

SEED = 23
PERM16 = [5, 0, 15, 9, 3, 12, 7, 1, 14, 2, 11, 8, 4, 13, 6, 10]
HOLES = [9, -1, 3, 15, -1, -1, 0, 12, 7]
GEOMETRY = {"init_prod_r": 4, "init_prod_bit0": -1}
MOVES = ("deferred", "realize_calls", "listed_launches")


def _fm_ops(c):
    from qcmrf_amd import ir
    mask = (1 << c["w"]) - 1
    for q in c["zero"]:
        mask &= ~(1 << q)
    tables = fm.tables_for(c["factors"], c["seed"], c["overrides"])
    return [ir.op_init(mask)] + [ir.op_diag(qs, t) for qs, t in zip(c["factors"], tables)]


def _engine(ops, w, devices=1, defer=1, **opts):
    from qcmrf_amd import _lib, program
    rec, data = program.encode(ops)
    eng = _lib.Engine(w, devices=(0,) * devices)
    for k, v in dict(opts, defer_state=defer).items():
        eng.set_option(k, v)
    eng.exec(rec, data)
    return eng, (rec, data)


def _moved(a, b):
    return (b["deferred"], b["realize_calls"] - a["realize_calls"], b["listed_launches"] - a["listed_launches"])


def _check(ops, w, runs, devices=1, defer=1, **opts):
    """every (shots, meas_qubits) of ``runs``: the ordered call, then the unordered one on the same handle -- the same
    multiset, the same movement of state_info; then the unordered call first on a freshly run program"""
    eng, prog = _engine(ops, w, devices, defer, **opts)
    try:
        assert eng.state_info()["deferred"] == bool(defer)
        for shots, meas in runs:
            i0 = eng.state_info()
            old = eng.sample(shots, SEED, meas)
            i1 = eng.state_info()
            new = eng.sample_unordered(shots, SEED, meas)
            i2 = eng.state_info()
            assert new.dtype == np.uint64 and new.shape == old.shape == (shots,)
            diff = int((np.sort(old) != np.sort(new)).sum())
            print("%d shots, meas %s: %d sorted words differ; state_info moved %s / %s"
                  % (shots, "all" if meas is None else len(meas), diff, _moved(i0, i1), _moved(i1, i2)))
            assert diff == 0
            assert _moved(i0, i1) == _moved(i1, i2), (i0, i1, i2)
            if shots > 64 and meas is None:
                assert not np.array_equal(old, np.sort(old))          # the ordered call still shuffles
        shots, meas = runs[0]
        want = np.sort(eng.sample(shots, SEED, meas))
        eng.exec(*prog)
        i0 = eng.state_info()
        assert np.array_equal(np.sort(eng.sample_unordered(shots, SEED, meas)), want)
        first = _moved(i0, eng.state_info())
        eng.exec(*prog)
        i0 = eng.state_info()
        eng.sample(shots, SEED, meas)
        assert first == _moved(i0, eng.state_info())
    finally:
        eng.close()


def test_chain_on_a_deferred_shard_every_shot_count():
    """W = 14, R = 4: 1, 2, 4096 shots and 70 000, past the 65 535 workgroups of the one-workgroup-per-shot launches"""
    _check(dc.default_ops(seed=2, zero=(13,), w=14), 14, [(4096, None), (1, None), (2, None), (70000, None)], **GEOMETRY)


def test_chain_on_a_deferred_shard_measurement_maps():
    _check(dc.default_ops(), dc.W, [(4096, PERM16), (4096, HOLES), (2, PERM16), (1, HOLES)], **GEOMETRY)


def test_chain_at_r6():
    c = fm.CASES["r6_bit-1"]
    _check(_fm_ops(c), c["w"], [(4096, None)], init_prod_r=6, init_prod_bit0=-1)


def test_stored_state():
    _check(dc.default_ops(), dc.W, [(4096, None), (4096, PERM16), (1, None)], defer=0)


def test_two_virtual_shards_take_the_host_walk():
    _check(dc.default_ops(seed=3, zero=()), dc.W, [(4096, None), (4096, HOLES), (2, None)], devices=2, **GEOMETRY)


def test_host_walk_by_option():
    _check(dc.default_ops(), dc.W, [(4096, None), (4096, HOLES), (1, None)], sample_chain=0, **GEOMETRY)
    _check(dc.default_ops(), dc.W, [(4096, PERM16)], defer=0, sample_chain=0)


@pytest.mark.parametrize("defer,fixed", [(1, {9: 1}), (1, {3: 1}), (0, {9: 0, 3: 1}), (1, {})], ids=["block_bit", "inner_bit", "stored", "no_mask"])
def test_post_selected(defer, fixed):
    """two engines in the same state, one call each (a conditioned call can realise the state it finds deferred): the same
    multiset and mass, and state_info ends the same"""
    fmask = sum(1 << q for q in fixed)
    fval = sum(v << q for q, v in fixed.items())
    ops = dc.default_ops(seed=7)
    e0, _ = _engine(ops, dc.W, defer=defer, post_select_list=1, **GEOMETRY)
    e1, _ = _engine(ops, dc.W, defer=defer, post_select_list=1, **GEOMETRY)
    try:
        for shots, meas in [(4096, None), (4096, HOLES), (1, None)]:
            old, m0 = e0.sample_cond(shots, SEED, meas, fmask, fval)
            new, m1 = e1.sample_cond_unordered(shots, SEED, meas, fmask, fval)
            assert m0 == m1 and m0 > 0
            assert np.array_equal(np.sort(old), np.sort(new))
            if meas is None:
                assert ((new & np.uint64(fmask)) == np.uint64(fval)).all()
            i0, i1 = e0.state_info(), e1.state_info()
            assert {k: i0[k] for k in MOVES} == {k: i1[k] for k in MOVES}, (i0, i1)
        none, m = e1.sample_cond_unordered(0, SEED, None, fmask, fval)
        assert none.shape == (0,) and m == m0
    finally:
        e0.close()
        e1.close()


def _error_of(call):
    with pytest.raises(Exception) as e:
        call()
    return type(e.value), str(e.value)


@pytest.mark.parametrize("chain", [0, 1])
def test_zero_norm_is_the_same_error(chain):
    factors = dc.random_factors(dc.W, [dc.REG_BIT], 6, seed=5)
    ops = dc.program_ops(dc.W, [dc.REG_BIT], factors, seed=6, tables={2: np.zeros(2 ** len(factors[2]))})
    eng, _ = _engine(ops, dc.W, sample_chain=chain, **GEOMETRY)
    try:
        a = _error_of(lambda: eng.sample(100, SEED))
        b = _error_of(lambda: eng.sample_unordered(100, SEED))
        assert a == b and a[0] is ValueError and "zero norm" in a[1], (a, b)
        a = _error_of(lambda: eng.sample(10, SEED, [dc.W]))
        b = _error_of(lambda: eng.sample_unordered(10, SEED, [dc.W]))                   # a measured qubit that does not exist
        assert a == b and a[0] is ValueError, (a, b)
    finally:
        eng.close()


def test_zero_mass_is_the_same_error():
    eng, _ = _engine(dc.default_ops(), dc.W, defer=0)                                    # qubit REG_BIT stays |0>
    try:
        bit = 1 << dc.REG_BIT
        a = _error_of(lambda: eng.sample_cond(100, SEED, None, bit, bit))
        b = _error_of(lambda: eng.sample_cond_unordered(100, SEED, None, bit, bit))
        assert a == b and a[0] is ValueError and "zero probability" in a[1], (a, b)
        a = _error_of(lambda: eng.sample_cond(100, SEED, None, 0b100, 0b110))
        b = _error_of(lambda: eng.sample_cond_unordered(100, SEED, None, 0b100, 0b110))
        assert a == b and a[0] is ValueError, (a, b)
        assert np.array_equal(np.sort(eng.sample(512, SEED)), np.sort(eng.sample_unordered(512, SEED)))   # still usable
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# through run(): the switch on and off
# ---------------------------------------------------------------------------------------------------------------------
def _run_both(circuit, **kw):
    from qcmrf_amd import backend as bk
    assert bk.native_counts_available(), "qcmrf_amd._counts_native is not built (python -m qcmrf_amd.build)"
    out = {}
    be = bk.QsvBackend()
    try:
        for on, path in ((True, "native"), (False, "python")):
            bk.use_native_counts(on)
            res = be.run(circuit, seed_simulator=1984, **kw).result()
            assert res.metadata(0)["counts_path"] == path
            out[path] = res.get_counts()
    finally:
        bk.use_native_counts(True)
        be.close()
    assert list(out["native"].items()) == list(out["python"].items())
    assert sum(out["native"].values()) == kw["shots"]
    return out["native"]


def test_run_config1():
    from qcmrf_amd import QCMRF
    g = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "config1.json")))
    counts = _run_both(QCMRF(g["cliques"], g["theta"]), shots=1024)
    assert all(len(k) == 8 for k in counts)


def test_run_chain9():
    from oracle import gate_stream as gs
    from qcmrf_amd import QCMRF
    counts = _run_both(QCMRF(gs.chain_cliques(9), (-np.linspace(0.05, 1.5, 32)).tolist()), shots=4096)
    assert all(len(k) == 18 for k in counts) and list(counts) == sorted(counts)


def test_run_post_select():
    from conftest import random_theta
    from qcmrf_amd import QCMRF, mrf
    cliques = [[0, 1], [1, 2], [2, 3]]
    qc = QCMRF(cliques, random_theta(mrf.dimension(cliques)))
    post = qc.post_selection()
    counts = _run_both(qc, shots=2048, post_select=post)
    assert all(k[len(k) - 1 - c] == str(v) for k in counts for c, v in post.items())


def test_run_noisy():
    from qcmrf_amd import QCMRF
    from qcmrf_amd.noise import NoiseModel, ReadoutError, depolarizing_error
    g = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "config1.json")))
    nm = NoiseModel()
    nm.add_all_qubit_quantum_error(depolarizing_error(0.02, 1), "h")
    nm.add_all_qubit_readout_error(ReadoutError([[0.97, 0.03], [0.05, 0.95]]))
    _run_both(QCMRF(g["cliques"], g["theta"], with_measurements=True), shots=3000, noise_model=nm)
