"""Conditional marginals for a batch of evidence rows, on the host: the helpers of tests/_rows_cases.py against each other,
``mrf.conditional_marginals`` against brute force, the planted mistakes, ``QCMRF.conditional_marginals`` / ``predict_proba``
/ ``QsvBackend.marginals_rows`` on the stand-in engine, ``learn.fit_incomplete``, and the build (header, export, binding)."""
import ctypes
import os
import re

import numpy as np
import pytest

import _marginal_cases as mc
import _rows_cases as rc
from conftest import random_theta
from qcmrf_amd import QCMRF, learn, mrf
from qcmrf_amd.backend import QsvBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def backend(**options):
    b = QsvBackend(**options)
    b._engine_factory = rc.factory
    return b


# ---- the row sets and the stand-in engine ---------------------------------------------------------------------------------------
def test_row_sets_cover_what_the_gpu_tests_say():
    assert sorted(len(f) for f in rc.ROWS_MIXED) == [0, 2, 3, 3, 11, 14]
    assert len({mc.mask_of(f)[0] for f in rc.ROWS_ONE_MASK}) == 1 and len({mc.mask_of(f)[1] for f in rc.ROWS_ONE_MASK}) == 8
    assert [len(f) for f in rc.ROWS_19] == [0, 2, 12, 19] and len(rc.GROUPS_19[-1]) == 8
    assert (1 << 19) // 4096 == 128                                           # the unfixed row: 128 chunks, two fold levels
    m, v = rc.masks_of(rc.ROWS_SHARDS)
    assert m == [(1 << 13) | (1 << 4), 1 << 13, (1 << 12) | (1 << 13) | 1, 0, (1 << 12) | (1 << 11)]
    assert all(x & ~y == 0 for x, y in zip(v, m))


def test_stand_in_engine_rows_are_its_single_calls_and_it_refuses_what_the_entry_point_refuses():
    eng = rc.RowsNumpyEngine(6, 1)
    rs = np.random.RandomState(3)
    amp = rs.standard_normal(64) + 1j * rs.standard_normal(64)
    eng.sh[0] = amp
    groups = [[1, 4], [], [0, 5, 2]]
    rows = [{}, {4: 1}, {0: 1, 5: 0}, {4: 1}]
    out, mass = eng.marginals_cond_rows(groups, *rc.masks_of(rows))
    assert out.shape == (4, 13) and eng.rows_calls == 1
    for r, f in enumerate(rows):
        flat, m = rc.single_flat(eng, groups, f)
        assert out[r].tobytes() == flat.tobytes() and mass[r] == m
    for masks, vals, text in (([], [], "0 rows"), ([0] * 65537, [0] * 65537, "65537 rows"), ([0, 0, 4], [0, 0, 6], "row 2"),
                              ([0, 1 << 6], [0, 0], "row 1")):
        with pytest.raises(ValueError) as e:
            eng.marginals_cond_rows(groups, masks, vals)
        assert text in str(e.value)
    with pytest.raises(ValueError):
        eng.marginals_cond_rows([[0, 0]], [0], [0])


# ---- mrf.conditional_marginals ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", sorted(rc.GRAPHS))
def test_mrf_conditional_marginals_against_brute_force(graph):
    cliques = rc.GRAPHS[graph]
    n = mrf.num_vertices(cliques)
    th = random_theta(mrf.dimension(cliques), scale=1.0, seed=21)
    rows = rc.all_rows(n)                                                     # 3^n: every observation pattern of every x
    assert rows.shape == (3 ** n, n)
    mu, pr = mrf.conditional_marginals(cliques, th, rows)
    bmu, bpr = rc.brute_conditionals(cliques, th, rows)
    assert mu.shape == (3 ** n, mrf.dimension(cliques)) and pr.shape == (3 ** n,)
    assert np.abs(mu - bmu).max() < 1e-13 and np.abs(pr - bpr).max() < 1e-13
    hidden = int(np.flatnonzero((rows == -1).all(axis=1))[0])
    assert np.abs(mu[hidden] - mrf.marginals(cliques, th)).max() < 1e-14 and abs(pr[hidden] - 1.0) < 1e-14
    full = (rows >= 0).all(axis=1)
    assert abs(pr[full].sum() - 1.0) < 1e-13                                   # the fully observed rows are the joint states
    assert np.isin(mu[full], (0.0, 1.0)).all()
    for beta in (0.6,):
        a = mrf.conditional_marginals(cliques, th, rows[::7], beta)
        b = rc.brute_conditionals(cliques, th, rows[::7], beta)
        assert np.abs(a[0] - b[0]).max() < 1e-13 and np.abs(a[1] - b[1]).max() < 1e-13


def test_mrf_conditional_marginals_refusals():
    cliques = rc.GRAPHS["chain4"]
    th = random_theta(12)
    for bad in ([[0, 1, -1]], [[0, 1, 2, -1]], [[0, 1, -2, 1]], [0, 1, 0, 1]):
        with pytest.raises(ValueError):
            mrf.conditional_marginals(cliques, th, np.array(bad))


@pytest.mark.parametrize("graph", sorted(rc.GRAPHS))
def test_the_model_of_the_device_result_is_the_host_value(graph):
    cliques = rc.GRAPHS[graph]
    th = random_theta(mrf.dimension(cliques), scale=1.0, seed=22)
    rows = rc.sampled_rows(cliques, th, 24, seed=5)
    mu, pr = rc.modelled_conditionals(cliques, th, rows)
    wmu, wpr = mrf.conditional_marginals(cliques, th, rows)
    assert np.abs(mu - wmu).max() < 1e-12 and np.abs(pr - wpr).max() < 1e-12


@pytest.mark.parametrize("mistake", rc.MISTAKES)
def test_every_planted_mistake_is_caught(mistake):
    caught = []
    for graph in sorted(rc.GRAPHS):
        cliques = rc.GRAPHS[graph]
        th = random_theta(mrf.dimension(cliques), scale=1.0, seed=22)
        rows = rc.sampled_rows(cliques, th, 24, seed=5)
        mu, pr = rc.modelled_conditionals(cliques, th, rows, mistake=mistake)
        wmu, wpr = mrf.conditional_marginals(cliques, th, rows)
        caught.append(not (np.abs(mu - wmu).max() < 1e-10 and np.abs(pr - wpr).max() < 1e-10))
    assert all(caught), (mistake, caught)


# ---- QCMRF.conditional_marginals / predict_proba / backend.marginals_rows on the stand-in engine -----------------------------------
@pytest.mark.parametrize("graph", sorted(rc.GRAPHS))
@pytest.mark.parametrize("options", [{}, {"fusion": 0}, {"devices": (0,) * 4}], ids=["default", "gate_by_gate", "four_shards"])
def test_qcmrf_conditional_marginals(graph, options):
    cliques = rc.GRAPHS[graph]
    n = mrf.num_vertices(cliques)
    th = random_theta(mrf.dimension(cliques))
    qc = QCMRF(cliques, th)
    x = rc.sampled_rows(cliques, th, 1, hidden=0.0, seed=9)[0]
    rows = rc.patterns_of(x)
    be = backend(**options)
    mu, pr, ps = qc.conditional_marginals(be, rows)
    assert be.last_engine.rows_calls == 1 and getattr(be.last_engine, "marginal_calls", 0) == 0     # ONE batched call
    wmu, wpr = mrf.conditional_marginals(cliques, th, rows)
    assert mu.shape == (2 ** n, qc.dimension) and pr.shape == (2 ** n,)
    assert np.abs(mu - wmu).max() < 1e-12 and np.abs(pr - wpr).max() < 1e-12
    assert abs(ps - mrf.success_probability(cliques, th)) < 1e-12
    assert np.abs(mu[0] - qc.marginals(be)[0]).max() < 1e-14                  # all hidden: the marginals themselves
    for v in range(n):
        pp = qc.predict_proba(be, rows, v)
        want = np.array([float(r[v]) if r[v] >= 0 else sum(wmu[i, j] for j in _ones(cliques, v)) for i, r in enumerate(rows)])
        assert np.abs(pp - want).max() < 1e-12


def _ones(cliques, v):
    """entries of mu, in the first clique that holds v, in which v is 1"""
    off = 0
    for C in cliques:
        if v in C:
            k = len(C)
            return [off + y for y in range(2 ** k) if (y >> (k - 1 - list(C).index(v))) & 1]
        off += 2 ** len(C)
    raise AssertionError(v)


def test_qcmrf_conditional_marginals_refusals_and_zero_rows():
    cliques = rc.GRAPHS["chain4"]
    th = random_theta(12)
    qc = QCMRF(cliques, th)
    be = backend()
    for bad in ([[0, 1, -1]], [[0, 1, 2, -1]], [0, 1, 0, 1]):
        with pytest.raises(ValueError):
            qc.conditional_marginals(be, np.array(bad))
    with pytest.raises(ValueError, match="no clique"):
        qc.predict_proba(be, np.array([[0, 1, -1, -1]]), 4)
    mu, pr, ps = qc.conditional_marginals(be, np.zeros((0, 4), dtype=int))      # no data rows: only the denominator's row
    assert mu.shape == (0, 12) and pr.shape == (0,) and abs(ps - mrf.success_probability(cliques, th)) < 1e-12

    class Zero(rc.RowsNumpyEngine):
        def marginals_cond_rows(self, groups, masks, vals):
            out, mass = super().marginals_cond_rows(groups, masks, vals)
            out[1], mass[1] = 0.0, 0.0
            return out, mass
    be = QsvBackend()
    be._engine_factory = lambda n, devices=(0,), rank=None, world_size=None: Zero(n, len(devices))
    with pytest.raises(ValueError, match="row 1"):
        qc.conditional_marginals(be, np.array([[0, 1, -1, -1], [1, 1, 0, -1], [-1, -1, -1, -1]]))


def test_backend_marginals_rows_maps_through_the_layout_and_refuses_as_marginals_does():
    be = backend()
    with pytest.raises(RuntimeError, match="run"):
        be.marginals_rows([[0]], [{}])
    qc = QCMRF(rc.GRAPHS["chain4"], random_theta(12))
    be = backend(devices=(0,) * 4)
    be.run(qc, shots=0)
    groups, rows = [[0, 5], [7, 2, 3], []], [{6: 0, 1: 1}, {}, {7: 1}, {6: 0, 1: 1}]
    out, mass = be.marginals_rows(groups, rows)
    for r, f in enumerate(rows):
        parts, m = be.marginals(groups, f)
        assert out[r].tobytes() == np.concatenate(parts).tobytes() and mass[r] == m

    class Two:
        world, rank = 2, 0
    be._last_comm = Two()
    with pytest.raises(ValueError, match="one process"):
        be.marginals_rows(groups, rows)
    be._last_comm = None
    with pytest.raises(ValueError):
        be.marginals_rows(groups, [])


# ---- learn.fit_incomplete ------------------------------------------------------------------------------------------------------------
def host_fn(cliques, beta=1.0):
    return lambda theta, rows: mrf.conditional_marginals(cliques, theta, rows, beta)


@pytest.mark.parametrize("graph", ["chain4", "triangles"])
def test_fit_incomplete_with_nothing_hidden_is_fit(graph):
    cliques = rc.GRAPHS[graph]
    star = np.asarray(random_theta(mrf.dimension(cliques), scale=1.0, seed=11))
    rows = rc.sampled_rows(cliques, star, 50, hidden=0.0, seed=2)
    mu_hat = mrf.empirical_marginals(cliques, rows)
    for steps in range(1, 9):                                                  # step by step
        a, ha = learn.fit_incomplete(cliques, rows, host_fn(cliques), steps=steps)
        b, hb = learn.fit(cliques, mu_hat, lambda th: mrf.marginals(cliques, th), steps=steps)
        assert np.abs(a - b).max() < 1e-12 and np.abs(np.array([g for _, g in ha]) - np.array(hb)).max() < 1e-12


@pytest.mark.parametrize("graph", ["chain4", "triangles"])
@pytest.mark.parametrize("beta", [1.0, 0.7])
def test_fit_incomplete_ascends_the_marginal_likelihood(graph, beta):
    cliques = rc.GRAPHS[graph]
    star = np.asarray(random_theta(mrf.dimension(cliques), scale=1.0, seed=11))
    rows = rc.sampled_rows(cliques, star, 64, hidden=0.3, seed=4, beta=beta)
    assert (rows == -1).any() and (rows >= 0).any()
    theta, hist = learn.fit_incomplete(cliques, rows, host_fn(cliques, beta), steps=30, beta=beta)
    ll = [l for l, _ in hist] + [float(np.log(mrf.conditional_marginals(cliques, theta, rows, beta)[1]).mean())]
    assert len(hist) == 30 and (theta <= 0).all()
    assert all(b >= a - 1e-12 for a, b in zip(ll, ll[1:])), np.diff(ll).min()
    assert ll[-1] > ll[0]
    with pytest.raises(ValueError):
        learn.fit_incomplete(cliques, rows, host_fn(cliques), theta0=np.zeros(3), steps=1)


def test_fit_incomplete_through_the_circuit_is_fit_incomplete_through_the_pmf():
    cliques = rc.GRAPHS["chain4"]
    star = np.asarray(random_theta(12, scale=1.0, seed=12))
    rows = rc.sampled_rows(cliques, star, 16, hidden=0.3, seed=6)
    be = backend()
    a, ha = learn.fit_incomplete(cliques, rows, learn.conditionals_on(be, cliques), steps=3)
    b, hb = learn.fit_incomplete(cliques, rows, host_fn(cliques), steps=3)
    assert np.abs(a - b).max() < 1e-9 and np.abs(np.array(ha) - np.array(hb)).max() < 1e-9


# ---- the build --------------------------------------------------------------------------------------------------------------------
def test_library_exports_and_header_declares_qsv_marginals_cond_rows():
    from qcmrf_amd import _lib, build
    lib = ctypes.CDLL(build.build(verbose=False))
    assert hasattr(lib, "qsv_marginals_cond_rows")
    assert "qsv_marginals_cond_rows" in _lib.SIGNATURES and len(_lib.SIGNATURES["qsv_marginals_cond_rows"][1]) == 9
    txt = open(os.path.join(ROOT, "include", "qsv.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"\bint\s+qsv_marginals_cond_rows\s*\(\s*qsv_handle\s*\*\s*h\s*,\s*int\s+n_groups\s*,", code)
    assert re.search(r"#define\s+QSV_MARG_MAX_ROWS\s+65536\b", txt)
    assert _lib.MARG_MAX_ROWS == rc.MAX_ROWS == 65536
    assert hasattr(_lib.Engine, "marginals_cond_rows")
    assert "marginals_rows" in txt
