"""qsv_marginals_cond against the exact reference (_marginal_cases.marginals_reference: one fsum per bin) on |amplitudes|^2
read back from the engine: stored states under every fix set and group set, bit-for-bit reproducibility from call to call
and for every number of workgroups, four virtual shards, implied zeros, deferred states (tiles listed, not realised),
the refusals, and ``QCMRF.marginals`` / ``learn.fit`` through the backend."""
import itertools
import math

import numpy as np
import pytest

import _deferred_cases as dc
import _marginal_cases as mc
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


def _flat(parts, mass):
    return np.concatenate(list(parts) + [np.array([mass])]).tobytes()


def _check(eng, p, groups, fixed, what=None):
    """one call against the reference: every bin, the contradicting bins, every group's total, the mass"""
    fm, fv = mc.mask_of(fixed)
    parts, mass = eng.marginals_cond(groups, fm, fv)
    want, want_mass = mc.marginals_reference(p, groups, fm, fv)
    assert len(parts) == len(groups)
    worst = 0.0
    for i, (grp, got, ref) in enumerate(zip(groups, parts, want)):
        assert got.dtype == np.float64 and got.shape == (1 << len(grp),)
        err = np.abs(got - ref)
        rel = float((err[ref > 0] / ref[ref > 0]).max()) if (ref > 0).any() else 0.0
        worst = max(worst, rel)
        assert (err <= SUM_SLACK * ref).all(), (what, i, grp, rel)
        assert (got[mc.contradicting_bins(grp, fixed)] == 0.0).all(), (what, i, grp)
        assert abs(math.fsum(got.tolist()) - mass) <= SUM_SLACK * mass, (what, i, grp)
    print("marginals %s: mass %.17g fsum %.17g, worst bin %.3g relative" % (what, mass, want_mass, worst))
    assert abs(mass - want_mass) <= SUM_SLACK * want_mass, what
    return parts, mass


# ---------------------------------------------------------------------------------------------------------------------
# stored state, 14 qubits
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stored_engine(lib):
    v, p = _stored()
    with lib.Engine(N) as eng:
        eng.set_amplitudes(0, v)
        yield eng, p


@pytest.mark.parametrize("gname", sorted(mc.GROUP_SETS))
@pytest.mark.parametrize("fname", sorted(mc.FIX_SETS))
def test_stored_state(stored_engine, fname, gname):
    eng, p = stored_engine
    fixed, groups = mc.FIX_SETS[fname], mc.GROUP_SETS[gname]
    eng.reset_stats()
    parts, mass = _check(eng, p, groups, fixed, "%s/%s" % (fname, gname))
    k = eng.stats()["kinds"]["prob"]
    assert k["launches"] == 1 and k["bytes"] == 16.0 * (1 << (N - len(fixed)))       # 2^-f of the shard is read, once
    fm, fv = mc.mask_of(fixed)
    _, smass = eng.sample_cond(0, 1, None, fm, fv)
    assert abs(mass - smass) <= SUM_SLACK * smass
    # the same call again: the same bytes, and nothing cached (a second pass)
    launches = eng.stats()["kinds"]["prob"]["launches"]
    again = eng.marginals_cond(groups, fm, fv)
    assert _flat(*again) == _flat(parts, mass)
    assert eng.stats()["kinds"]["prob"]["launches"] == launches + 1


@pytest.mark.parametrize("fname", ["none", "strided", "contiguous_blocks"])
def test_the_grid_changes_no_bit(stored_engine, fname):
    """4, 2 and 4 compact blocks: one workgroup walks them all, three share them, or one each"""
    eng, p = stored_engine
    fm, fv = mc.mask_of(mc.FIX_SETS[fname])
    try:
        got = {}
        for grid in (0, 1, 3):
            eng.set_option("marginals_grid", grid)
            got[grid] = [_flat(*eng.marginals_cond(mc.GROUP_SETS[g], fm, fv)) for g in sorted(mc.GROUP_SETS)]
        assert got[1] == got[0] and got[3] == got[0]
    finally:
        eng.set_option("marginals_grid", 0)


def test_the_grid_changes_no_bit_64_blocks(lib):
    """18 qubits, nothing fixed: 64 compact blocks, by five workgroups (thirteen chunks for the first four) and by 64"""
    v, p = _stored(18, 45)
    groups = mc.GROUP_SETS["pairs"] + [[17, 0, 12], [16], [15, 11, 3, 8, 13, 17, 2, 6]]
    with lib.Engine(18) as eng:
        eng.set_amplitudes(0, v)
        parts, mass = _check(eng, p, groups, {}, "18 qubits")
        eng.set_option("marginals_grid", 5)
        assert _flat(*eng.marginals_cond(groups)) == _flat(parts, mass)
        fixed = {17: 1, 4: 0}
        eng.set_option("marginals_grid", 0)
        parts, mass = _check(eng, p, groups, fixed, "18 qubits, 16 blocks")
        eng.set_option("marginals_grid", 5)
        assert _flat(*eng.marginals_cond(groups, *mc.mask_of(fixed))) == _flat(parts, mass)


# ---------------------------------------------------------------------------------------------------------------------
# four virtual shards (L = 12)
# ---------------------------------------------------------------------------------------------------------------------
SHARD_CASES = {
    "group_on_shard_bit": ({3: 1}, [[13, 2], [12], [5, 12, 13, 0], [1, 2]]),
    "fixed_shard_bit": ({13: 1, 4: 0}, [[0, 1], [11, 7, 3]]),
    "both": ({12: 0, 11: 1}, [[13, 12, 11, 0], [12], [13], [6, 13]]),
}


@pytest.mark.parametrize("name", sorted(SHARD_CASES))
def test_four_virtual_shards(lib, name):
    fixed, groups = SHARD_CASES[name]
    v, p = _stored(N, 42)
    with lib.Engine(N, devices=(0,) * 4) as eng:
        eng.set_amplitudes(0, v)
        eng.reset_stats()
        parts, mass = _check(eng, p, groups, fixed, name)
        fm, fv = mc.mask_of(fixed)
        # the reference shard by shard, with hi: what each shard owes
        L = N - 2
        per = [mc.marginals_reference(p[s << L:(s + 1) << L], groups, fm, fv, hi=s << L) for s in range(4)]
        live = [s for s in range(4) if ((s << L) & fm) == (fv & ~((1 << L) - 1))]
        assert all(per[s][1] == 0.0 for s in range(4) if s not in live)
        assert eng.stats()["kinds"]["prob"]["launches"] == len(live)         # a shard that disagrees with a fixed shard bit is skipped
        for i in range(len(groups)):
            ref = sum(per[s][0][i] for s in live)                            # up to four exact sums added: within 4 ulp of exact
            assert (np.abs(parts[i] - ref) <= SUM_SLACK * ref + 4 * np.spacing(ref)).all()


# ---------------------------------------------------------------------------------------------------------------------
# implied zeros
# ---------------------------------------------------------------------------------------------------------------------
def test_implied_zeros(lib):
    W, zero = 16, [15]
    ops = dc.program_ops(W, zero, dc.random_factors(W, zero, 10, seed=3), seed=103)
    groups = [[15, 0], [14, 15, 3], [2, 8], [], [13, 14]]
    cases = [{15: 0, 3: 1, 9: 0}, {2: 1, 8: 0}, {13: 1, 14: 0}, {}]
    e1 = dc.start(ops, 0, W, implied_zeros=1)
    e0 = dc.start(ops, 0, W, implied_zeros=0)
    try:
        p = sc.probs(e0.amplitudes())
        for fixed in cases:
            a = _check(e1, p, groups, fixed, "implied zeros %s" % fixed)
            b = _check(e0, p, groups, fixed, "zeros written %s" % fixed)
            for x, y in zip(a[0], b[0]):
                assert (np.abs(x - y) <= 2 * SUM_SLACK * y).all()
        parts, mass = e1.marginals_cond(groups, 1 << 15, 1 << 15)            # the zero half alone
        assert mass == 0.0 and all(not x.any() for x in parts)
    finally:
        e0.close()
        e1.close()


# ---------------------------------------------------------------------------------------------------------------------
# deferred states, W = 16: lane bits 0..4 and 11, wave bits 5 and 6, block bits 7..10, register bits 12..15
# ---------------------------------------------------------------------------------------------------------------------
GEOMETRY = {"init_prod_r": 4, "init_prod_bit0": -1}
DEFERRED_GROUPS = [[q, q + 1] for q in range(15)] + [[9, 0, 15], [], [14, 3, 10, 7]]


def _pair(seed, **opts):
    ops = dc.default_ops(seed=seed)
    e0, e1 = dc.start(ops, 0, **GEOMETRY, **opts), dc.start(ops, 1, **GEOMETRY, **opts)
    assert e1.state_info()["deferred"] and not e0.state_info()["deferred"]
    return e0, e1


@pytest.mark.parametrize("fixed", [{dc.BLOCK_BIT: 1}, {dc.BLOCK_BIT: 0, 3: 1}, {7: 1, 10: 0, 14: 1}], ids=["9", "9_3", "7_10_14"])
def test_deferred_state_lists_the_tiles(lib, fixed):
    e0, e1 = _pair(7, post_select_list=1)
    try:
        fm, fv = mc.mask_of(fixed)
        before = e1.state_info()
        got = e1.marginals_cond(DEFERRED_GROUPS, fm, fv)
        after = e1.state_info()
        assert after["deferred"] and after["realize_calls"] == before["realize_calls"] == 0, after
        assert after["listed_launches"] == before["listed_launches"] + 1, after
        want = _check(e0, sc.probs(e0.amplitudes()), DEFERRED_GROUPS, fixed, "stored %s" % fixed)
        assert _flat(*got) == _flat(*want)
        again = e1.marginals_cond(DEFERRED_GROUPS, fm, fv)                   # nothing cached: listed again, the same bytes
        assert _flat(*again) == _flat(*want) and e1.state_info()["listed_launches"] == before["listed_launches"] + 2
        dc.same(e0.amplitudes(), e1.amplitudes())
    finally:
        e0.close()
        e1.close()


@pytest.mark.parametrize("fixed", [{dc.REG_BIT: 0}, {dc.THREAD_BIT: 1}, {}], ids=["register_bit", "thread_bit", "nothing"])
def test_deferred_state_is_realised_without_a_block_bit(lib, fixed):
    e0, e1 = _pair(8, post_select_list=1)
    try:
        fm, fv = mc.mask_of(fixed)
        got = e1.marginals_cond(DEFERRED_GROUPS, fm, fv)
        info = e1.state_info()
        assert not info["deferred"] and info["realize_calls"] == 1 and info["listed_launches"] == 0, info
        want = _check(e0, sc.probs(e0.amplitudes()), DEFERRED_GROUPS, fixed, "stored %s" % fixed)
        assert _flat(*got) == _flat(*want)
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
    bad = [
        ([], 0, 0, "groups"),
        ([[0]] * 65, 0, 0, "65 groups"),
        ([[0], list(range(9))], 0, 0, "group 1"),
        ([list(range(8))] * 16 + [[]], 0, 0, "4097 bins"),
        ([[0, 1], [2, N]], 0, 0, "group 1: qubit %d" % N),
        ([[0], [1], [5, 3, 5]], 0, 0, "group 2: qubit 5 repeated"),
        ([[0]], 0b100, 0b110, "fix_val"),
        ([[0]], 1 << N, 0, "qubit %d" % N),
    ]
    for groups, fm, fv, text in bad:
        with pytest.raises(ValueError) as e:
            eng.marginals_cond(groups, fm, fv)
        assert text in str(e.value), (text, str(e.value))
    L = lib.load()
    out, k, q = (C.c_double * 2)(), (C.c_int * 1)(1), (C.c_int * 1)(0)
    for args in ((None, 1, k, q, 0, 0, out, None), (eng._h, 1, None, q, 0, 0, out, None), (eng._h, 1, k, None, 0, 0, out, None),
                 (eng._h, 1, k, q, 0, 0, None, None)):
        assert L.qsv_marginals_cond(*args) == -1 and b"NULL" in L.qsv_last_error()
    _check(eng, p, mc.GROUP_SETS["pairs"], mc.FIX_SETS["mixed"], "after the refusals")


# ---------------------------------------------------------------------------------------------------------------------
# the model level
# ---------------------------------------------------------------------------------------------------------------------
GRAPHS = {"chain4": [[0, 1], [1, 2], [2, 3]], "triangles": [[0, 1, 2], [2, 3, 4]], "k4": [[0, 1, 2, 3]]}


@pytest.mark.parametrize("graph", sorted(GRAPHS))
@pytest.mark.parametrize("how", ["default", "gate_by_gate", "lowered", "loop"])
def test_qcmrf_marginals(lib, graph, how):
    from qcmrf_amd import QCMRF, mrf
    from qcmrf_amd.backend import QsvBackend
    cliques = GRAPHS[graph]
    th = random_theta(mrf.dimension(cliques))
    qc = QCMRF(cliques, th)
    be = QsvBackend()
    try:
        if how == "lowered":
            from qcmrf_amd.transpile import transpile
            mu, ps = qc.marginals(be, circuit=transpile(qc, basis_gates=['cx', 'id', 'rz', 'sx', 'x']))
        else:
            mu, ps = qc.marginals(be, **({"fusion": 0} if how == "gate_by_gate" else {}))
        want = mrf.marginals(cliques, th)
        print("QCMRF.marginals %s %s: max error %.3g, success error %.3g" % (graph, how, np.abs(mu - want).max(),
                                                                         abs(ps - mrf.success_probability(cliques, th))))
        assert mu.dtype == np.float64 and np.abs(mu - want).max() < 1e-10
        assert abs(ps - mrf.success_probability(cliques, th)) < 1e-10
        if how == "loop":
            off = 0
            for C in cliques:
                for i, y in enumerate(itertools.product([0, 1], repeat=len(C))):
                    e, s1 = qc.expectation_sufficient_statistic(be, C, y)
                    assert abs(mu[off + i] - e) < 1e-12, (C, y)
                off += 2 ** len(C)
    finally:
        be.close()


def test_qcmrf_marginals_keeps_a_deferred_state_deferred(lib):
    from qcmrf_amd import QCMRF, mrf
    from qcmrf_amd.backend import QsvBackend
    cliques = [[i, i + 1] for i in range(7)]               # 16 qubits: wide enough for the generator to defer its state
    th = random_theta(mrf.dimension(cliques))
    be = QsvBackend(engine_options={"defer_state": 1, "post_select_list": 1})
    try:
        mu, ps = QCMRF(cliques, th).marginals(be)
        info = be.last_engine.state_info()
        assert info["deferred"] and info["realize_calls"] == 0, info
        assert np.abs(mu - mrf.marginals(cliques, th)).max() < 1e-10
        assert abs(ps - mrf.success_probability(cliques, th)) < 1e-10
    finally:
        be.close()


def test_qcmrf_marginals_of_the_whole_state(lib):
    from qcmrf_amd import QCMRF, mrf
    from qcmrf_amd.backend import QsvBackend
    cliques = GRAPHS["triangles"]
    n = 5
    qc = QCMRF(cliques, random_theta(mrf.dimension(cliques)))
    be = QsvBackend()
    try:
        mu, ps = qc.marginals(be, post_selected=False)
        pw = sc.probs(be.statevector())
    finally:
        be.close()
    assert abs(ps - 1.0) < 1e-12
    groups = [[n - 1 - v for v in reversed(C)] for C in cliques]
    want, mass = mc.marginals_reference(pw, groups, 0, 0)
    assert np.abs(mu - np.concatenate(want) / mass).max() < 1e-12


def test_fit_on_the_device_is_fit_on_the_host(lib):
    from qcmrf_amd import learn, mrf
    from qcmrf_amd.backend import QsvBackend
    cliques = GRAPHS["chain4"]
    mu_hat = mrf.marginals(cliques, random_theta(12, scale=1.0, seed=12))
    be = QsvBackend()
    try:
        a, ha = learn.fit(cliques, mu_hat, learn.marginals_on(be, cliques), steps=3)
    finally:
        be.close()
    b, hb = learn.fit(cliques, mu_hat, lambda th: mrf.marginals(cliques, th), steps=3)
    print("fit: max theta difference %.3g" % np.abs(a - b).max())
    assert np.abs(a - b).max() < 1e-9
