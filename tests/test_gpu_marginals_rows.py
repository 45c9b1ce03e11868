"""qsv_marginals_cond_rows against qsv_marginals_cond, byte for byte (``tobytes()``), on the same engine state: mixed masks
in one batch, one mask with every value, every composition of the batch, every grid and slab size, both fold levels in
one work list, four virtual shards, implied zeros, deferred states (tiles listed once for the common condition, or
realised once), the refusals, and ``QCMRF.conditional_marginals`` / ``predict_proba`` / ``learn.fit_incomplete`` through
the backend."""
import math

import numpy as np
import pytest

import _deferred_cases as dc
import _marginal_cases as mc
import _rows_cases as rc
import _sampler_cases as sc
from conftest import random_theta

pytestmark = pytest.mark.gpu

SUM_SLACK = mc.SUM_SLACK
N = mc.N


@pytest.fixture(scope="module")
def lib():
    from qcmrf_amd import _lib
    _lib.load()
    assert _lib.device_count() >= 1
    return _lib


_STATE = {}


def _stored(n=N, seed=41):
    if (n, seed) not in _STATE:
        v = sc.rand_state(n, seed)
        v.setflags(write=False)
        _STATE[n, seed] = (v, sc.probs(v))
    return _STATE[n, seed]


def _rows(eng, groups, rows):
    out, mass = eng.marginals_cond_rows(groups, *rc.masks_of(rows))
    assert out.dtype == np.float64 and out.shape == (len(rows), rc.nbins(groups)) and mass.shape == (len(rows),)
    return out, mass


def _singles(eng, groups, rows):
    return [rc.single_flat(eng, groups, f) for f in rows]


def _same_bytes(out, mass, singles, what=None):
    for r, (flat, m) in enumerate(singles):
        assert out[r].tobytes() == flat.tobytes(), (what, r, float(np.abs(out[r] - flat).max()))
        assert np.float64(mass[r]).tobytes() == np.float64(m).tobytes(), (what, r, mass[r], m)


def _against_reference(p, groups, fixed, flat, mass, what=None):
    want, want_mass = mc.marginals_reference(p, groups, *mc.mask_of(fixed))
    off = 0
    for i, (grp, ref) in enumerate(zip(groups, want)):
        got = flat[off:off + (1 << len(grp))]
        assert (np.abs(got - ref) <= SUM_SLACK * ref).all(), (what, i, grp)
        assert (got[mc.contradicting_bins(grp, fixed)] == 0.0).all(), (what, i, grp)
        off += 1 << len(grp)
    assert abs(mass - want_mass) <= SUM_SLACK * want_mass, what


def _nc(n_local, fixed):
    return 1 << (n_local - sum(1 for q in fixed if q < n_local))


# ---------------------------------------------------------------------------------------------------------------------
# stored state, 14 qubits
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stored_engine(lib):
    v, p = _stored()
    with lib.Engine(N) as eng:
        eng.set_amplitudes(0, v)
        yield eng, p


def _mixed(eng, p, gname):
    groups, rows = mc.GROUP_SETS[gname], rc.ROWS_MIXED
    singles = _singles(eng, groups, rows)
    eng.reset_stats()
    out, mass = _rows(eng, groups, rows)
    k = eng.stats()["kinds"]["prob"]
    assert k["launches"] == 1 and k["bytes"] == 16.0 * sum(_nc(N, f) for f in rows), k
    _same_bytes(out, mass, singles, gname)
    for r, f in enumerate(rows):
        _against_reference(p, groups, f, out[r], mass[r], (gname, r))
    return out, mass


@pytest.mark.parametrize("gname", sorted(mc.GROUP_SETS))
def test_mixed_masks_in_one_batch(stored_engine, gname):
    eng, p = stored_engine
    _mixed(eng, p, gname)


def test_one_mask_every_value(stored_engine):
    eng, p = stored_engine
    groups = mc.GROUP_SETS["with_fixed"]
    out, mass = _rows(eng, groups, rc.ROWS_ONE_MASK)
    _same_bytes(out, mass, _singles(eng, groups, rc.ROWS_ONE_MASK))
    norm = math.fsum(p.tolist())
    assert abs(math.fsum(mass.tolist()) - norm) <= SUM_SLACK * norm


@pytest.mark.parametrize("gname", ["pairs", "with_fixed"])
def test_composition_changes_no_byte(stored_engine, gname):
    eng, p = stored_engine
    groups, rows = mc.GROUP_SETS[gname], rc.ROWS_MIXED
    singles = _singles(eng, groups, rows)
    rev = list(range(len(rows)))[::-1]
    out, mass = _rows(eng, groups, [rows[r] for r in rev])
    _same_bytes(out, mass, [singles[r] for r in rev], "reversed")
    rep = [0, 3, 1, 3, 2, 3, 4, 5]
    out, mass = _rows(eng, groups, [rows[r] for r in rep])
    _same_bytes(out, mass, [singles[r] for r in rep], "row 3 three times")
    for r in range(len(rows)):
        out, mass = _rows(eng, groups, [rows[r]])
        _same_bytes(out, mass, [singles[r]], "row %d alone" % r)


def test_grid_and_slab_size_change_no_byte(stored_engine):
    eng, p = stored_engine
    groups, rows = mc.GROUP_SETS["mixed_k"], rc.ROWS_MIXED
    singles = _singles(eng, groups, rows)
    B = len(rows)
    try:
        for grid in (0, 1, 3):
            for slab in (0, 1, 2, 5):
                eng.set_option("marginals_grid", grid)
                eng.set_option("marginals_rows", slab)
                eng.reset_stats()
                out, mass = _rows(eng, groups, rows)
                _same_bytes(out, mass, singles, (grid, slab))
                assert eng.stats()["kinds"]["prob"]["launches"] == (1 if slab == 0 else -(-B // slab)), (grid, slab)
        with pytest.raises(ValueError):
            eng.set_option("marginals_rows", -1)
    finally:
        eng.set_option("marginals_grid", 0)
        eng.set_option("marginals_rows", 0)


def test_heterogeneous_work_list_with_both_fold_levels(lib):
    """19 qubits: 128 chunks (two fold levels), 32 blocks, 32 entries and one entry in one work list"""
    v, p = _stored(19, 46)
    with lib.Engine(19) as eng:
        eng.set_amplitudes(0, v)
        singles = _singles(eng, rc.GROUPS_19, rc.ROWS_19)
        eng.reset_stats()
        out, mass = _rows(eng, rc.GROUPS_19, rc.ROWS_19)
        k = eng.stats()["kinds"]["prob"]
        assert k["launches"] == 1 and k["bytes"] == 16.0 * sum(_nc(19, f) for f in rc.ROWS_19)
        _same_bytes(out, mass, singles)
        _against_reference(p, rc.GROUPS_19, {}, out[0], mass[0], "19 qubits, nothing fixed")
        eng.set_option("marginals_grid", 7)
        out, mass = _rows(eng, rc.GROUPS_19, rc.ROWS_19[::-1])
        _same_bytes(out, mass, singles[::-1], "seven workgroups, reversed")


# ---------------------------------------------------------------------------------------------------------------------
# four virtual shards (L = 12)
# ---------------------------------------------------------------------------------------------------------------------
def test_four_virtual_shards(lib):
    groups = [[13, 12, 11, 0], [12], [13], [6, 13]]                           # SHARD_CASES["both"] of test_gpu_marginals.py
    rows = rc.ROWS_SHARDS
    v, p = _stored(N, 42)
    L = N - 2
    with lib.Engine(N, devices=(0,) * 4) as eng:
        eng.set_amplitudes(0, v)
        singles = _singles(eng, groups, rows)
        eng.reset_stats()
        out, mass = _rows(eng, groups, rows)
        _same_bytes(out, mass, singles)
        live = [[s for s in range(4) if ((s << L) & m) == (x & ~((1 << L) - 1))] for m, x in zip(*rc.masks_of(rows))]
        assert [len(l) for l in live] == [2, 2, 1, 4, 2]
        k = eng.stats()["kinds"]["prob"]
        assert k["launches"] == len(set().union(*live)) == 4
        assert k["bytes"] == 16.0 * sum(len(l) * _nc(L, f) for l, f in zip(live, rows))
        eng.reset_stats()
        out, mass = _rows(eng, groups, [rows[0], rows[2]])                     # both fix shard bit 13 to 1: shards 2 and 3
        _same_bytes(out, mass, [singles[0], singles[2]])
        assert eng.stats()["kinds"]["prob"]["launches"] == 2


# ---------------------------------------------------------------------------------------------------------------------
# implied zeros
# ---------------------------------------------------------------------------------------------------------------------
def test_implied_zeros(lib):
    W, zero = 16, [15]
    ops = dc.program_ops(W, zero, dc.random_factors(W, zero, 10, seed=3), seed=103)
    groups = [[15, 0], [14, 15, 3], [2, 8], [], [13, 14]]
    rows = rc.ROWS_IMPLIED
    e1 = dc.start(ops, 0, W, implied_zeros=1)
    e0 = dc.start(ops, 0, W, implied_zeros=0)
    try:
        a, am = _rows(e1, groups, rows)
        _same_bytes(a, am, _singles(e1, groups, rows), "implied zeros")
        b, bm = _rows(e0, groups, rows)
        _same_bytes(b, bm, _singles(e0, groups, rows), "zeros written")
        assert not a[-1].any() and am[-1] == 0.0 and not np.signbit(a[-1]).any() and not np.signbit(am[-1])
        assert (np.abs(a - b) <= 2 * SUM_SLACK * b).all() and (np.abs(am - bm) <= 2 * SUM_SLACK * bm).all()
    finally:
        e0.close()
        e1.close()


# ---------------------------------------------------------------------------------------------------------------------
# deferred states, W = 16 (geometry and pairs as in test_gpu_marginals.py)
# ---------------------------------------------------------------------------------------------------------------------
GEOMETRY = {"init_prod_r": 4, "init_prod_bit0": -1}
DEFERRED_GROUPS = [[q, q + 1] for q in range(15)] + [[9, 0, 15], [], [14, 3, 10, 7]]


def _pair(seed, **opts):
    ops = dc.default_ops(seed=seed)
    e0, e1 = dc.start(ops, 0, **GEOMETRY, **opts), dc.start(ops, 1, **GEOMETRY, **opts)
    assert e1.state_info()["deferred"] and not e0.state_info()["deferred"]
    return e0, e1


def test_deferred_state_lists_the_tiles_once(lib):
    assert dc.BLOCK_BIT == 9
    rows = [{9: 1}, {9: 1, 3: 1}, {9: 1, 7: 1, 14: 0}, {9: 1, 0: 0, 15: 1}]
    e0, e1 = _pair(7, post_select_list=1)
    try:
        before = e1.state_info()
        out, mass = _rows(e1, DEFERRED_GROUPS, rows)
        after = e1.state_info()
        assert after["deferred"] and after["realize_calls"] == before["realize_calls"] == 0, after
        assert after["listed_launches"] == before["listed_launches"] + 1, after
        _same_bytes(out, mass, _singles(e0, DEFERRED_GROUPS, rows))
        dc.same(e0.amplitudes(), e1.amplitudes())
    finally:
        e0.close()
        e1.close()


@pytest.mark.parametrize("rows", [[{9: 1}, {9: 0}], [{9: 1}, {}], [{dc.REG_BIT: 0, 9: 1}, {dc.REG_BIT: 0, 9: 0}],
                                  [{dc.THREAD_BIT: 1, 8: 1}, {dc.THREAD_BIT: 1}]],
                         ids=["no_common_value", "one_row_unfixed", "register_bit", "thread_bit"])
def test_deferred_state_is_realised_once(lib, rows):
    e0, e1 = _pair(8, post_select_list=1)
    try:
        out, mass = _rows(e1, DEFERRED_GROUPS, rows)
        info = e1.state_info()
        assert not info["deferred"] and info["realize_calls"] == 1 and info["listed_launches"] == 0, info
        _same_bytes(out, mass, _singles(e0, DEFERRED_GROUPS, rows))
        dc.same(e0.amplitudes(), e1.amplitudes())
    finally:
        e0.close()
        e1.close()


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_engine_usable(lib, stored_engine):
    import ctypes as C
    eng, p = stored_engine
    g1 = [[0]]
    bad = [
        (g1, [], [], "0 rows"),
        (g1, [0] * 65537, [0] * 65537, "65537 rows"),
        (g1, [0, 0, 0b100], [0, 0, 0b110], "row 2"),
        (g1, [0, 1 << N], [0, 0], "row 1"),
        ([], [0], [0], "groups"),
        ([[0]] * 65, [0], [0], "65 groups"),
        ([[0], list(range(9))], [0], [0], "group 1"),
        ([list(range(8))] * 16 + [[]], [0], [0], "4097 bins"),
        ([[0, 1], [2, N]], [0], [0], "group 1: qubit %d" % N),
        ([[0], [1], [5, 3, 5]], [0], [0], "group 2: qubit 5 repeated"),
    ]
    for groups, masks, vals, text in bad:
        with pytest.raises(ValueError) as e:
            eng.marginals_cond_rows(groups, masks, vals)
        assert text in str(e.value), (text, str(e.value))
    with pytest.raises(ValueError) as e:
        eng.marginals_cond_rows(g1, [0, 0, 0b100], [0, 0, 0b110])
    assert "fix_val" in str(e.value)
    L = lib.load()
    out, ms, k, q = (C.c_double * 4)(), (C.c_double * 2)(), (C.c_int * 1)(1), (C.c_int * 1)(0)
    m, v = (C.c_uint64 * 2)(0, 1), (C.c_uint64 * 2)(0, 0)
    for args in ((None, 1, k, q, 2, m, v, out, ms), (eng._h, 1, None, q, 2, m, v, out, ms), (eng._h, 1, k, None, 2, m, v, out, ms),
                 (eng._h, 1, k, q, 2, None, v, out, ms), (eng._h, 1, k, q, 2, m, None, out, ms), (eng._h, 1, k, q, 2, m, v, None, ms)):
        assert L.qsv_marginals_cond_rows(*args) == -1 and b"NULL" in L.qsv_last_error()
    assert L.qsv_marginals_cond_rows(eng._h, 1, k, q, 2, m, v, out, None) == 0            # mass may be NULL
    _mixed(eng, p, sorted(mc.GROUP_SETS)[0])


# ---------------------------------------------------------------------------------------------------------------------
# the model level
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", sorted(rc.GRAPHS))
@pytest.mark.parametrize("how", ["default", "gate_by_gate", "lowered"])
def test_qcmrf_conditional_marginals(lib, graph, how):
    from qcmrf_amd import QCMRF, mrf
    from qcmrf_amd.backend import QsvBackend
    cliques = rc.GRAPHS[graph]
    n = mrf.num_vertices(cliques)
    th = random_theta(mrf.dimension(cliques))
    qc = QCMRF(cliques, th)
    x = rc.sampled_rows(cliques, th, 1, hidden=0.0, seed=9)[0]
    rows = rc.patterns_of(x)                                                  # all hidden first, fully observed last
    be = QsvBackend()
    try:
        if how == "lowered":
            from qcmrf_amd.transpile import transpile
            opts = {"circuit": transpile(qc, basis_gates=['cx', 'id', 'rz', 'sx', 'x'])}
        else:
            opts = {"fusion": 0} if how == "gate_by_gate" else {}
        mu, pr, ps = qc.conditional_marginals(be, rows, **opts)
        k = be.last_engine.stats()["kinds"]["prob"]
        wmu, wpr = mrf.conditional_marginals(cliques, th, rows)
        print("QCMRF.conditional_marginals %s %s: mu %.3g, p_rows %.3g, success %.3g, prob launches %d" % (
            graph, how, np.abs(mu - wmu).max(), np.abs(pr - wpr).max(), abs(ps - mrf.success_probability(cliques, th)), k["launches"]))
        assert mu.dtype == np.float64 and mu.shape == wmu.shape and np.abs(mu - wmu).max() < 1e-10
        assert np.abs(pr - wpr).max() < 1e-10
        assert abs(ps - mrf.success_probability(cliques, th)) < 1e-10
        # the whole row set costs the launches of ONE query: what QCMRF.marginals books for its single condition (the run
        # resets the stats; norm() books the same in both), and the batched call by itself is exactly one launch
        qc.marginals(be, **opts)
        assert be.last_engine.stats()["kinds"]["prob"]["launches"] == k["launches"]
        W = n + len(cliques) + 1
        anc = {q: 0 for q in range(n, W)}
        fixed_rows = [{**anc, **{n - 1 - v: int(r[v]) for v in range(n) if r[v] >= 0}} for r in rows] + [anc]
        be.last_engine.reset_stats()
        out, mass = be.marginals_rows([[n - 1 - v for v in reversed(C)] for C in cliques], fixed_rows)
        assert be.last_engine.stats()["kinds"]["prob"]["launches"] == 1
        assert np.abs(out[:-1] / mass[:-1, None] - wmu).max() < 1e-10 and np.abs(mass[:-1] / mass[-1] - wpr).max() < 1e-10
        for v in (0, n - 1):
            pp = qc.predict_proba(be, rows, v, **opts)
            want = np.array([float(r[v]) if r[v] >= 0 else wmu[i, _ones(cliques, v)].sum() for i, r in enumerate(rows)])
            assert np.abs(pp - want).max() < 1e-10
    finally:
        be.close()


def _ones(cliques, v):
    off = 0
    for C in cliques:
        if v in C:
            k = len(C)
            return [off + y for y in range(2 ** k) if (y >> (k - 1 - list(C).index(v))) & 1]
        off += 2 ** len(C)
    raise AssertionError(v)


def test_qcmrf_conditional_marginals_keeps_a_deferred_state_deferred(lib):
    from qcmrf_amd import QCMRF, mrf
    from qcmrf_amd.backend import QsvBackend
    cliques = [[i, i + 1] for i in range(7)]               # 16 qubits: wide enough for the generator to defer its state
    th = random_theta(mrf.dimension(cliques))
    rows = rc.sampled_rows(cliques, th, 40, hidden=0.3, seed=13)
    be = QsvBackend(engine_options={"defer_state": 1, "post_select_list": 1})
    try:
        qc = QCMRF(cliques, th)
        # what the run itself lists (run(shots=0, post_select=...) takes a mass pass of its own for the metadata)
        listed = []
        for _ in range(2):
            be.run(qc, shots=0, post_select=qc.post_selection())
            listed.append(be.last_engine.state_info()["listed_launches"])
        per_run = listed[1] - listed[0]
        mu, pr, ps = qc.conditional_marginals(be, rows)
        info = be.last_engine.state_info()
        assert info["deferred"] and info["realize_calls"] == 0, info
        assert info["listed_launches"] == listed[1] + per_run + 1, (info, listed)     # ONE listed launch for the 41 conditions
        wmu, wpr = mrf.conditional_marginals(cliques, th, rows)
        assert np.abs(mu - wmu).max() < 1e-10 and np.abs(pr - wpr).max() < 1e-10
        assert abs(ps - mrf.success_probability(cliques, th)) < 1e-10
    finally:
        be.close()


def test_fit_incomplete_on_the_device_is_fit_incomplete_on_the_host(lib):
    from qcmrf_amd import learn, mrf
    from qcmrf_amd.backend import QsvBackend
    cliques = rc.GRAPHS["chain4"]
    star = np.asarray(random_theta(12, scale=1.0, seed=12))
    rows = rc.sampled_rows(cliques, star, 64, hidden=0.3, seed=6)
    be = QsvBackend()
    try:
        a, ha = learn.fit_incomplete(cliques, rows, learn.conditionals_on(be, cliques), steps=3)
    finally:
        be.close()
    b, hb = learn.fit_incomplete(cliques, rows, lambda th, rw: mrf.conditional_marginals(cliques, th, rw), steps=3)
    print("fit_incomplete: max theta difference %.3g" % np.abs(a - b).max())
    assert np.abs(a - b).max() < 1e-9
