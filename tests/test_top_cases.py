"""The most probable states on the host: the exact reference of ``qsv_top_cond`` (_top_cases.top_reference) told apart
from five planted mistakes, the state builders of the GPU tests, ``mrf.map_states`` against brute force,
``QsvBackend.top_states`` / ``QCMRF.map_states`` through a numpy stand-in for the engine, ``run_experiment --map``, the
condition on the models the GPU tests use, and the build (header, export, binding)."""
import ctypes
import itertools
import json
import os
import re

import numpy as np
import pytest

import _top_cases as tc
from conftest import ROOT, random_theta
from qcmrf_amd import QCMRF, mrf
from qcmrf_amd.backend import QsvBackend
from qcmrf_amd.workloads import REFERENCE_GRAPHS, chain


def backend(**options):
    b = QsvBackend(**options)
    b._engine_factory = tc.factory
    return b


def same(a, b):
    return all(np.asarray(x).dtype == np.asarray(y).dtype and np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


# ---- the reference and the planted mistakes ---------------------------------------------------------------------------------
def brute_top(amps, k, fix_mask, fix_val, hi):
    """the contract spelled out entry by entry in Python floats"""
    c = []
    for i, a in enumerate(np.asarray(amps, dtype=np.complex128)):
        x = i + hi
        p = a.real * a.real + a.imag * a.imag
        if (x & fix_mask) == fix_val and p > 0:
            c.append((-p, x))
    c.sort()
    return [x for _, x in c[:k]], [-p for p, _ in c[:k]]


@pytest.mark.parametrize("name", [c[0] for c in tc.CASES])
def test_reference_is_the_contract_and_the_blockwise_selection(name):
    _, amps, k, fixed, hi = [c for c in tc.CASES if c[0] == name][0]
    fm, fv = tc.mask_of(fixed)
    x, p = tc.top_reference(amps, k, fm, fv, hi)
    bx, bp = brute_top(amps, k, fm, fv, hi)
    assert x.dtype == np.uint64 and p.dtype == np.float64
    assert x.tolist() == bx and p.tolist() == bp
    assert (p > 0).all() and ((x & np.uint64(fm)) == np.uint64(fv)).all()
    for block in (1, 3, 16, 1 << 20):                                  # whatever the blocks: a pure function of the state
        assert same(tc.top_planted(amps, k, fm, fv, hi, None, block), (x, p)), block


@pytest.mark.parametrize("mistake", tc.MISTAKES)
def test_every_planted_mistake_fails_a_case(mistake):
    caught = []
    for name, amps, k, fixed, hi in tc.CASES:
        fm, fv = tc.mask_of(fixed)
        if not same(tc.top_planted(amps, k, fm, fv, hi, mistake), tc.top_reference(amps, k, fm, fv, hi)):
            caught.append(name)
    print("%s: caught by %s" % (mistake, caught))
    assert caught, mistake


def test_reference_with_hi_is_the_shard_of_the_whole():
    amps = tc.random_state(8, 11)
    fm, fv = tc.mask_of({7: 1, 2: 0})
    whole = tc.top_reference(amps, 6, fm, fv)
    parts = [tc.top_reference(amps[s << 6:(s + 1) << 6], 6, fm, fv, hi=s << 6) for s in range(4)]
    assert parts[0][0].size == 0 and parts[1][0].size == 0             # shards 0, 1 disagree with qubit 7 = 1
    x = np.concatenate([pt[0] for pt in parts])
    p = np.concatenate([pt[1] for pt in parts])
    order = np.lexsort((x, -p))[:6]
    assert same((x[order], p[order]), whole)


def test_reference_drops_nan_and_zero():
    amps = np.array([0.5, np.nan, 0.0, 0.25, np.nan + 1j, 1e-170], dtype=np.complex128)
    x, p = tc.top_reference(amps, 6, 0, 0)
    assert x.tolist() == [0, 3] and p.tolist() == [0.25, 0.0625]


def test_builders():
    w = 13
    for name, a in (("ascending", tc.ascending(w)), ("descending", tc.descending(w)), ("sawtooth", tc.sawtooth(w))):
        p = tc.weights(a)
        d = np.diff(p)
        if name == "ascending":
            assert (d > 0).all()
        elif name == "descending":
            assert (d < 0).all()
        else:
            inner = np.arange(1, 1 << w) % tc.BLOCK != 0
            assert (d[inner] > 0).all() and (d[~inner] < 0).all() and p[:tc.BLOCK].min() > p[tc.BLOCK:].max()
    for t in range(w):
        a, want = tc.two_maxima(w, 4321, t)
        x, p = tc.top_reference(a, 3, 0, 0)
        assert x.tolist() == want and p[0] == p[1] == 1.0 and p[2] == 0.875 * 0.875
    a, at = tc.equal_maxima(w, 65)
    x, p = tc.top_reference(a, 64, 0, 0)
    assert np.array_equal(x, at[:64]) and (p == 1.0).all()
    a, want = tc.tiny_weights(w)
    x, p = tc.top_reference(a, 8, 0, 0)
    assert x.tolist() == want and 0 < p[-1] < 2.3e-308
    assert sum(1 for _ in tc.F10) == 10 and all(max(m, default=0) < tc.N for m in tc.MASKS.values())


# ---- mrf.map_states ---------------------------------------------------------------------------------------------------------
def brute_map(cliques, theta, k, beta, evidence):
    n = mrf.num_vertices(cliques)
    rows = []
    for x in itertools.product([0, 1], repeat=n):
        if any(x[v] != b for v, b in (evidence or {}).items()):
            continue
        lp, off = 0.0, 0
        for C in cliques:
            lp += theta[off + int("".join(str(x[v]) for v in C), 2)]
            off += 2 ** len(C)
        rows.append((np.exp(beta * lp), int("".join(map(str, x)), 2), x))
    Z = sum(r[0] for r in rows)
    rows.sort(key=lambda r: (-r[0], r[1]))
    return np.array([r[2] for r in rows[:k]]), np.array([r[0] / Z for r in rows[:k]])


@pytest.mark.parametrize("g", [2, 5, 6])                          # a chain, two triangles, a 4-clique
def test_mrf_map_states_against_brute_force(g):
    cliques = REFERENCE_GRAPHS[g]
    n = mrf.num_vertices(cliques)
    th = random_theta(mrf.dimension(cliques), seed=50 + g)
    for k, beta, ev in ((1, 1.0, None), (5, 0.7, {0: 1}), (3, 1.0, {n - 1: 0, 1: 1}), (2 ** n + 3, 1.0, None)):
        x, p = mrf.map_states(cliques, th, k=k, beta=beta, evidence=ev)
        bx, bp = brute_map(cliques, th, k, beta, ev)
        assert x.shape == (min(k, 2 ** (n - len(ev or {}))), n) and np.issubdtype(x.dtype, np.integer)
        assert np.array_equal(x, bx) and np.abs(p - bp).max() < 1e-14
        assert (np.diff(p) <= 0).all()
    full, pf = mrf.map_states(cliques, th, k=2 ** n)
    assert abs(pf.sum() - 1.0) < 1e-13
    # ties: the uniform model returns ascending xid
    x, p = mrf.map_states(cliques, np.zeros(mrf.dimension(cliques)), k=4, evidence={0: 1})
    assert np.array_equal(x, mrf.states_of(np.arange(4) + 2 ** (n - 1), n))
    with pytest.raises(ValueError):
        mrf.map_states(cliques, th, k=1, evidence={n: 0})
    with pytest.raises(ValueError):
        mrf.map_states(cliques, th, k=0)


# ---- the condition on the models of the GPU tests -------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(tc.MODELS))
def test_model_gaps(name):
    cliques, seed, evidence = tc.MODELS[name]
    th = random_theta(mrf.dimension(cliques), seed=seed)
    for ev in (None, evidence):
        _, p = mrf.map_states(cliques, th, k=max(tc.MODEL_KS) + 1, evidence=ev)
        gaps = p[:-1] - p[1:]
        print("%s %s: smallest gap among the top %d: %.3g" % (name, ev, p.size, gaps.min()))
        for k in tc.MODEL_KS:
            assert tc.gaps_ok(p, k), (name, ev, k)


# ---- QsvBackend.top_states / QCMRF.map_states on the stand-in engine ------------------------------------------------------------
@pytest.mark.parametrize("options", [{}, {"fusion": 0}, {"devices": (0,) * 4}], ids=["default", "gate_by_gate", "four_shards"])
def test_backend_top_states_maps_through_the_layout(options):
    cliques = chain(4)
    qc = QCMRF(cliques, random_theta(12, seed=21))
    be = backend(**{k: v for k, v in options.items() if k == "devices"})
    be.run(qc, shots=0, **{k: v for k, v in options.items() if k != "devices"})
    lay = list(be.last_plan.layout)
    logical = be.statevector()
    for k, fixed in ((1, None), (7, {6: 0, 1: 1}), (64, {4: 0, 5: 0, 6: 0, 7: 0}), (64, {q: 0 for q in range(3, 8)})):
        x, p = be.top_states(k, fixed)
        wx, wp = tc.top_reference(logical, k, *tc.mask_of(fixed or {}))
        assert x.dtype == np.uint64 and p.dtype == np.float64
        assert np.array_equal(x, wx) and same((p,), (wp,)), (lay, k, fixed)
    print("layout", lay)


def test_backend_top_states_under_a_permuted_layout():
    """a layout that is not the identity: the mask goes out physical, the indices come back logical, sorted by
    (-p, logical index)"""
    qc = QCMRF(chain(4), random_theta(12, seed=22))
    be = backend()
    be.run(qc, shots=0)
    eng, plan = be.last_engine, be.last_plan
    W = len(plan.layout)
    perm = [(q * 3 + 1) % W for q in range(W)]                         # W = 8: 3 is a unit mod 8
    assert sorted(perm) == list(range(W)) and perm != list(range(W))

    class Plan:
        layout = perm

    class Permuted:
        """an engine that stores ``logical`` with logical qubit q on physical bit perm[q]"""

        def __init__(self, logical):
            idx = np.arange(logical.size)
            at = np.zeros_like(idx)
            for q, b in enumerate(perm):
                at |= ((idx >> q) & 1) << b
            self.phys = np.zeros(logical.size, dtype=np.complex128)
            self.phys[at] = logical

        def top_cond(self, k, fm=0, fv=0):
            self.args = (k, fm, fv)
            return tc.top_reference(self.phys, k, fm, fv)
    logical = np.asarray(be.statevector(), dtype=np.complex128)
    tied = np.zeros(1 << W, dtype=np.complex128)
    tied[[3, 6, 200]] = [0.5, 0.5j, 0.25]                              # 3 -> physical 26, 6 -> physical 146: ascending either way ...
    tied2 = np.zeros(1 << W, dtype=np.complex128)
    tied2[[8, 128]] = [0.5, 0.5j]                                      # ... 8 -> physical 4 (perm[3] = 2), 128 -> physical 64 (perm[7] = 6)
    tied3 = np.zeros(1 << W, dtype=np.complex128)
    tied3[[4, 32]] = [0.5, 0.5j]                                       # 4 -> perm[2] = 7: physical 128; 32 -> perm[5] = 0: physical 1
    try:
        be.last_plan = Plan()
        be.last_engine = Permuted(logical)
        fixed = {7: 0, 2: 1}
        x, p = be.top_states(9, fixed)
        assert be.last_engine.args == (9, (1 << perm[7]) | (1 << perm[2]), 1 << perm[2])
        wx, wp = tc.top_reference(logical, 9, *tc.mask_of(fixed))
        assert np.array_equal(x, wx) and same((p,), (wp,))
        be.last_engine = Permuted(tied)
        x, p = be.top_states(3)
        assert x.tolist() == [3, 6, 200] and p.tolist() == [0.25, 0.25, 0.0625]
        be.last_engine = Permuted(tied3)                               # physical order reversed: re-sorted by logical index
        x, p = be.top_states(2)
        assert x.tolist() == [4, 32]
        x, p = be.top_states(1)                                        # a tie AT the k-th place: the physical order decides
        assert x.tolist() == [32]
    finally:
        be.last_engine, be.last_plan = eng, plan


def test_backend_top_states_refusals():
    be = backend()
    with pytest.raises(RuntimeError, match="run"):
        be.top_states(1)
    be.run(QCMRF(chain(3), random_theta(8)), shots=0)

    class Two:
        world, rank = 2, 0
    be._last_comm = Two()
    with pytest.raises(ValueError, match="one process"):
        be.top_states(1)
    be._last_comm = None
    for k in (0, 65):
        with pytest.raises(ValueError):
            be.top_states(k)
    x, p = be.top_states(2)
    assert x.size == 2


def p_evidence(cliques, th, evidence):
    n = mrf.num_vertices(cliques)
    p, _ = mrf.gibbs_pmf(cliques, th)
    m, val = mrf._evidence_mask(n, evidence)
    xid = np.arange(p.size)
    return float(p[(xid & m) == val].sum())


@pytest.mark.parametrize("name", ["chain3", "triangle", "k4"])
@pytest.mark.parametrize("options", [{}, {"fusion": 0}, {"devices": (0,) * 4}], ids=["default", "gate_by_gate", "four_shards"])
def test_qcmrf_map_states_closed_form(name, options):
    cliques, seed, evidence = tc.MODELS[name]
    th = random_theta(mrf.dimension(cliques), seed=seed)
    for with_m in (True, False):
        qc = QCMRF(cliques, th, with_measurements=with_m)
        for k in tc.MODEL_KS:
            for ev in (None, evidence):
                be = backend(**options)
                x, p, pc = qc.map_states(be, k=k, evidence=ev)
                wx, wp = mrf.map_states(cliques, th, k=k, evidence=ev)
                assert np.array_equal(x, wx) and x.shape == wx.shape and np.issubdtype(x.dtype, np.integer)
                assert np.abs(p - wp).max() < 1e-12
                assert abs(pc - mrf.success_probability(cliques, th) * p_evidence(cliques, th, ev)) < 1e-12
                assert be.last_engine.top_calls == 1 and be.last_engine.marginal_calls == 1
    # the MAP state is the mode of the exact pmf
    p, _ = mrf.gibbs_pmf(cliques, th)
    x, _, _ = QCMRF(cliques, th).map_states(backend())
    assert int("".join(map(str, x[0])), 2) == int(np.argmax(p))


def test_qcmrf_map_states_refusals():
    cliques = chain(3)
    qc = QCMRF(cliques, random_theta(8))

    class Never:
        def run(self, *a, **k):
            raise AssertionError("refused before anything runs")
    for bad in ({"k": 65}, {"k": 0}, {"evidence": {3: 1}}, {"evidence": {-1: 0}}):
        with pytest.raises(ValueError):
            qc.map_states(Never(), **bad)


# ---- run_experiment ---------------------------------------------------------------------------------------------------------
def test_run_experiment_map(tmp_path, monkeypatch, capsys):
    from qcmrf_amd import backend as be_mod, run_experiment
    import qcmrf_amd.workloads as wl
    monkeypatch.setattr(wl, "REFERENCE_GRAPHS", wl.REFERENCE_GRAPHS[:3])
    graphs = wl.REFERENCE_GRAPHS
    b = backend()
    monkeypatch.setattr(be_mod.Aer, "get_backend", lambda name="qasm_simulator", **o: b)
    args = ["--scale", "0.5", "--shots", "20", "--reps", "2", "--outdir", str(tmp_path), "--seed-simulator", "5", "--map", "3"]
    run_experiment.main(args)
    rows = json.load(open(tmp_path / "map_simulation_0.5.json"))
    models = json.load(open(tmp_path / "models_0.5.json"))
    assert len(rows) == 6
    i = 0
    for j, C in enumerate(graphs):
        for rep in range(2):
            th = models["THETAS"][str(j)][rep]
            wx, wp = mrf.map_states(C, th, k=3)
            assert tc.gaps_ok(mrf.map_states(C, th, k=4)[1], 3)
            assert sorted(rows[i]) == ["p", "success", "x"]
            assert rows[i]["x"] == wx.tolist()
            assert np.abs(np.array(rows[i]["p"]) - wp).max() < 1e-12
            assert abs(rows[i]["success"] - mrf.success_probability(C, th)) < 1e-12
            i += 1
    for noise in (["--readout", "0.02"], ["--depolarizing", "0.001,0.01"], ["--method", "density_matrix"]):
        with pytest.raises(SystemExit):
            run_experiment.main(args + noise)
        err = capsys.readouterr().err
        assert "--map" in err and "density_matrix" in err and "get_probabilities" in err
    with pytest.raises(SystemExit):
        run_experiment.main(args[:-1] + ["65"])
    assert "1..64" in capsys.readouterr().err


# ---- the build --------------------------------------------------------------------------------------------------------------
def test_library_exports_and_header_declares_qsv_top_cond():
    from qcmrf_amd import _lib, build
    lib = ctypes.CDLL(build.build(verbose=False))
    assert hasattr(lib, "qsv_top_cond")
    assert "qsv_top_cond" in _lib.SIGNATURES and len(_lib.SIGNATURES["qsv_top_cond"][1]) == 7
    txt = open(os.path.join(ROOT, "include", "qsv.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"\bint\s+qsv_top_cond\s*\(\s*qsv_handle\s*\*\s*h\s*,\s*int\s+k\s*,", code)
    assert re.search(r"#define\s+QSV_TOP_MAX_K\s+64\b", txt)
    assert mrf.MAP_MAX_K == _lib.TOP_MAX_K == tc.MAX_K == 64
    assert hasattr(_lib.Engine, "top_cond")
