"""qsv_top_cond against the exact reference (_top_cases.top_reference) on the amplitudes read back from the same engine:
indices compared with ==, weights bit for bit.  Random states under every mask and k, adversarial orders, ties, denormal
and underflowing weights, every top_grid, four virtual shards, implied zeros, deferred states (tiles listed, not
realised), the stats, the refusals, and ``QCMRF.map_states`` through the backend against ``mrf.map_states``."""
import ctypes as C

import numpy as np
import pytest

import _deferred_cases as dc
import _top_cases as tc
from conftest import random_theta

pytestmark = pytest.mark.gpu

N = tc.N


@pytest.fixture(scope="module")
def lib():
    from qcmrf_amd import _lib
    _lib.load()
    assert _lib.device_count() >= 1
    return _lib


def _same(got, want, what=None):
    (gx, gp), (wx, wp) = got, want
    assert gx.dtype == np.uint64 and gp.dtype == np.float64, what
    assert gx.shape == wx.shape and (gx == wx).all(), (what, gx[:8], wx[:8])
    assert gp.tobytes() == wp.astype(np.float64).tobytes(), (what, gp[:8], wp[:8])


def _check(eng, amps, k, fixed, what=None):
    """one call against the reference on ``amps`` (read back from ``eng``)"""
    fm, fv = tc.mask_of(fixed)
    got = eng.top_cond(k, fm, fv)
    want = tc.top_reference(amps, k, fm, fv)
    _same(got, want, (what, k, fixed))
    return got


class Planted:
    """one 14-qubit engine for the module; a case plants its amplitudes and reads them back once"""

    def __init__(self, lib):
        self.eng = lib.Engine(N)
        self.name = None
        self.amps = None

    def plant(self, name, make):
        if self.name != name:
            self.eng.set_amplitudes(0, make())
            self.amps = self.eng.amplitudes()
            self.amps.setflags(write=False)
            self.name = name
        return self.eng, self.amps


@pytest.fixture(scope="module")
def planted(lib):
    p = Planted(lib)
    yield p
    p.eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# random states
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", tc.KS)
@pytest.mark.parametrize("mask", sorted(tc.MASKS))
def test_random_state(planted, mask, k):
    eng, amps = planted.plant("random", lambda: tc.random_state(N, 41))
    fixed = tc.MASKS[mask]
    eng.reset_stats()
    x, p = _check(eng, amps, k, fixed, mask)
    assert x.size == min(k, 1 << (N - len(fixed)))                       # every weight of a random state is > 0
    st = eng.stats()["kinds"]["prob"]
    assert st["launches"] == 1 and st["bytes"] == 16.0 * (1 << (N - len(fixed)))     # 2^-f of the shard is read, once
    assert (np.diff(p) <= 0).all()
    again = eng.top_cond(k, *tc.mask_of(fixed))                          # nothing cached: a second pass, the same arrays
    _same(again, (x, p))
    assert eng.stats()["kinds"]["prob"]["launches"] == 2


def test_fewer_candidates_than_k(lib):
    with lib.Engine(4) as eng:
        eng.set_amplitudes(0, tc.random_state(4, 43))
        x, p = _check(eng, eng.amplitudes(), 64, {})
        assert x.size == 16
        x, p = _check(eng, eng.amplitudes(), 64, {1: 1})
        assert x.size == 8


# ---------------------------------------------------------------------------------------------------------------------
# adversarial orders: correctness cases, every block (or none after the first) brings entrants
# ---------------------------------------------------------------------------------------------------------------------
ORDERS = {"ascending": lambda: tc.ascending(N), "descending": lambda: tc.descending(N), "sawtooth": lambda: tc.sawtooth(N)}


@pytest.mark.parametrize("order", sorted(ORDERS))
def test_adversarial_order(planted, order):
    eng, amps = planted.plant(order, ORDERS[order])
    p = tc.weights(amps)
    assert np.unique(p).size == p.size
    for mask in ("none", "lane_bit", "register_bit", "block_bit", "mixed"):
        for k in tc.KS:
            x, _ = _check(eng, amps, k, tc.MASKS[mask], order)
            assert x.size == k
    if order == "ascending":
        assert eng.top_cond(3)[0].tolist() == [(1 << N) - 1, (1 << N) - 2, (1 << N) - 3]


# ---------------------------------------------------------------------------------------------------------------------
# ties
# ---------------------------------------------------------------------------------------------------------------------
def test_uniform_state_returns_the_lowest_indices(planted):
    eng = planted.eng
    planted.name = None
    eng.init_uniform((1 << N) - 1)
    amps = eng.amplitudes()
    for mask in sorted(tc.MASKS):
        fixed = tc.MASKS[mask]
        fm, fv = tc.mask_of(fixed)
        match = np.flatnonzero((np.arange(1 << N) & fm) == fv).astype(np.uint64)
        for k in tc.KS:
            x, p = _check(eng, amps, k, fixed, mask)
            assert np.array_equal(x, match[:k]) and np.unique(p).size == 1


def test_two_equal_maxima_on_every_compact_bit(planted):
    eng = planted.eng
    planted.name = None
    for t in range(N):
        a, want = tc.two_maxima(N, 4321 + 97 * t, t)
        eng.set_amplitudes(0, a)
        amps = eng.amplitudes()
        for k in (2, 3, 64):
            x, p = _check(eng, amps, k, {}, "bit %d" % t)
            assert x[:3].tolist() == want[:min(k, 3)] and p[0] == p[1]
        x, _ = _check(eng, amps, 1, {}, "bit %d" % t)
        assert x.tolist() == want[:1]


def test_65_equal_maxima_drop_the_highest_index(planted):
    made = {}

    def make():
        made["a"], made["at"] = tc.equal_maxima(N, 65)
        return made["a"]
    planted.name = None
    eng, amps = planted.plant("65 maxima", make)
    x, p = _check(eng, amps, 64, {})
    assert np.array_equal(x, made["at"][:64]) and (p == 1.0).all()
    for grid in (1, 3):                                                  # the 65 lie in all four blocks
        eng.set_option("top_grid", grid)
        _same(eng.top_cond(64), (x, p), grid)
    eng.set_option("top_grid", 0)


# ---------------------------------------------------------------------------------------------------------------------
# weights: a denormal, squares that underflow, an empty sub-cube; entries past n_found untouched
# ---------------------------------------------------------------------------------------------------------------------
def test_tiny_weights(lib, planted):
    made = {}

    def make():
        made["a"], made["want"] = tc.tiny_weights(N)
        return made["a"]
    planted.name = None
    eng, amps = planted.plant("tiny", make)
    x, p = _check(eng, amps, 8, {})
    assert x.tolist() == made["want"] and 0.0 < p[-1] < 2.3e-308         # the denormal comes last; the underflowed are not returned
    _check(eng, amps, 2, {})
    # the sub-cube with bit 0 clear holds only zeros and underflowed squares
    x, p = _check(eng, amps, 8, {0: 0, 1: 1})
    assert x.size == 0
    L = lib.load()
    idx = (C.c_uint64 * 8)(*[0xDEAD] * 8)
    pp = (C.c_double * 8)(*[-7.0] * 8)
    n = C.c_int(-1)
    assert L.qsv_top_cond(eng._h, 8, 0, 0, idx, pp, C.byref(n)) == 0
    assert n.value == 3 and list(idx)[:3] == made["want"] and list(idx)[3:] == [0xDEAD] * 5 and list(pp)[3:] == [-7.0] * 5
    assert L.qsv_top_cond(eng._h, 8, 3, 2, idx, pp, C.byref(n)) == 0
    assert n.value == 0 and list(idx)[:3] == made["want"] and list(pp)[3:] == [-7.0] * 5


def test_all_zero_state(lib):
    with lib.Engine(13) as eng:
        eng.set_amplitudes(0, np.zeros(1 << 13, dtype=np.complex128))
        x, p = eng.top_cond(64)
        assert x.size == 0 and p.size == 0


# ---------------------------------------------------------------------------------------------------------------------
# top_grid: no bit of the result depends on it
# ---------------------------------------------------------------------------------------------------------------------
GRIDS = (1, 2, 3, 7)


@pytest.mark.parametrize("state", ["random", "ascending", "sawtooth"])
def test_the_grid_changes_nothing(planted, state):
    make = ORDERS.get(state, lambda: tc.random_state(N, 41))
    eng, amps = planted.plant(state, make)
    try:
        for mask in ("none", "register_bit", "block_bit"):
            for k in (1, 17, 64):
                eng.set_option("top_grid", 0)
                want = _check(eng, amps, k, tc.MASKS[mask], state)
                for grid in GRIDS:
                    eng.set_option("top_grid", grid)
                    _same(eng.top_cond(k, *tc.mask_of(tc.MASKS[mask])), want, (state, mask, k, grid))
    finally:
        eng.set_option("top_grid", 0)


def test_the_grid_changes_nothing_64_blocks(lib):
    """18 qubits, nothing fixed: 64 compact blocks by one workgroup each, by 1, 2, 3 and 7; one fixed bit: 32 blocks"""
    with lib.Engine(18) as eng:
        for name, a in (("random", tc.random_state(18, 45)), ("ascending", tc.ascending(18))):
            eng.set_amplitudes(0, a)
            amps = eng.amplitudes()
            for fixed in ({}, {17: 1, 4: 0}):
                eng.set_option("top_grid", 0)
                want = _check(eng, amps, 64, fixed, name)
                for grid in GRIDS:
                    eng.set_option("top_grid", grid)
                    _same(eng.top_cond(64, *tc.mask_of(fixed)), want, (name, fixed, grid))
        with pytest.raises(ValueError):
            eng.set_option("top_grid", -1)


def test_the_grid_changes_nothing_128_blocks(lib):
    """19 qubits, nothing fixed: 128 workgroups' lists are merged in two launches (runs of 32 lists first), 64 and fewer in
    one; the same arrays"""
    with lib.Engine(19) as eng:
        for name, a in (("random", tc.random_state(19, 46)), ("descending", tc.descending(19))):
            eng.set_amplitudes(0, a)
            amps = eng.amplitudes()
            for k in (1, 64):
                eng.set_option("top_grid", 0)
                want = _check(eng, amps, k, {}, name)
                for grid in (64, 65, 97, 7):
                    eng.set_option("top_grid", grid)
                    _same(eng.top_cond(k), want, (name, k, grid))


# ---------------------------------------------------------------------------------------------------------------------
# four virtual shards (L = 12)
# ---------------------------------------------------------------------------------------------------------------------
def test_four_virtual_shards(lib):
    L = N - 2
    a = tc.background(N, 44)
    winners = [(3 << L) + 17, (0 << L) + 4000, (2 << L) + 1, (1 << L) + 2222, (3 << L) + 4095, (2 << L) + 2048]
    for r, w in enumerate(winners):
        a[w] = 1.0 - r / 16.0
    a[(1 << L) + 5] = a[(2 << L) + 5] = 0.5j                              # a tie across shards
    with lib.Engine(N, devices=(0,) * 4) as eng:
        eng.set_amplitudes(0, a)
        amps = eng.amplitudes()
        eng.reset_stats()
        x, p = _check(eng, amps, 8, {})
        assert x.tolist() == winners + [(1 << L) + 5, (2 << L) + 5]
        st = eng.stats()["kinds"]["prob"]
        assert st["launches"] == 4 and st["bytes"] == 4 * 16.0 * (1 << L)
        for fixed, live in (({13: 1}, 2), ({12: 0, 5: 0}, 2), ({13: 1, 12: 0, 0: 1}, 1)):
            eng.reset_stats()
            for k in (1, 5, 64):
                x, p = _check(eng, amps, k, fixed)
                fm, fv = tc.mask_of(fixed)
                assert x.size == k and ((x & np.uint64(fm)) == np.uint64(fv)).all()
            st = eng.stats()["kinds"]["prob"]                             # a shard that disagrees with a fixed shard bit is skipped
            nl = sum(1 for q in fixed if q < L)
            assert st["launches"] == 3 * live and st["bytes"] == 3 * live * 16.0 * (1 << (L - nl))
        x, _ = _check(eng, amps, 3, {13: 1})
        assert x.tolist() == [winners[0], winners[2], winners[4]]         # the indices carry the shard bits
        # shard by shard: what each shard owes, merged by the same order
        parts = [tc.top_reference(amps[s << L:(s + 1) << L], 64, 0, 0, hi=s << L) for s in range(4)]
        xs, ps = np.concatenate([q[0] for q in parts]), np.concatenate([q[1] for q in parts])
        order = np.lexsort((xs, -ps))[:64]
        _same(eng.top_cond(64), (xs[order], ps[order]))


# ---------------------------------------------------------------------------------------------------------------------
# implied zeros
# ---------------------------------------------------------------------------------------------------------------------
def test_implied_zeros(lib):
    W, zero = 16, [15]
    ops = dc.program_ops(W, zero, dc.random_factors(W, zero, 10, seed=3), seed=103)
    e1 = dc.start(ops, 0, W, implied_zeros=1)
    e0 = dc.start(ops, 0, W, implied_zeros=0)
    try:
        amps = e0.amplitudes()
        for fixed in ({15: 0, 3: 1, 9: 0}, {2: 1, 8: 0}, {13: 1, 14: 0}, {}):
            for k in (1, 64):
                a = _check(e1, amps, k, fixed, "implied zeros %s" % fixed)
                b = _check(e0, amps, k, fixed, "zeros written %s" % fixed)
                _same(a, b)
        for e in (e0, e1):
            x, p = e.top_cond(64, 1 << 15, 1 << 15)                       # the zero half alone
            assert x.size == 0
    finally:
        e0.close()
        e1.close()


# ---------------------------------------------------------------------------------------------------------------------
# deferred states, W = 16: lane bits 0..4 and 11, wave bits 5 and 6, block bits 7..10, register bits 12..15
# ---------------------------------------------------------------------------------------------------------------------
GEOMETRY = {"init_prod_r": 4, "init_prod_bit0": -1}


def _pair(seed, **opts):
    ops = dc.default_ops(seed=seed)
    e0, e1 = dc.start(ops, 0, **GEOMETRY, **opts), dc.start(ops, 1, **GEOMETRY, **opts)
    assert e1.state_info()["deferred"] and not e0.state_info()["deferred"]
    return e0, e1


@pytest.mark.parametrize("fixed", [{dc.BLOCK_BIT: 1}, {dc.BLOCK_BIT: 0, 3: 1}, {7: 1, 10: 0, 14: 1}], ids=["9", "9_3", "7_10_14"])
def test_deferred_state_lists_the_tiles(lib, fixed):
    e0, e1 = _pair(7, post_select_list=1)
    try:
        fm, fv = tc.mask_of(fixed)
        before = e1.state_info()
        got = e1.top_cond(64, fm, fv)
        after = e1.state_info()
        assert after["deferred"] and after["realize_calls"] == before["realize_calls"] == 0, after
        assert after["listed_launches"] == before["listed_launches"] + 1, after
        want = _check(e0, e0.amplitudes(), 64, fixed, "stored %s" % fixed)
        _same(got, want)
        _same(e1.top_cond(1, fm, fv), (want[0][:1], want[1][:1]))         # nothing cached: listed again
        assert e1.state_info()["listed_launches"] == before["listed_launches"] + 2 and e1.state_info()["deferred"]
        dc.same(e0.amplitudes(), e1.amplitudes())
    finally:
        e0.close()
        e1.close()


@pytest.mark.parametrize("fixed", [{dc.REG_BIT: 0}, {dc.THREAD_BIT: 1}, {}], ids=["register_bit", "thread_bit", "nothing"])
def test_deferred_state_is_realised_without_a_block_bit(lib, fixed):
    e0, e1 = _pair(8, post_select_list=1)
    try:
        fm, fv = tc.mask_of(fixed)
        got = e1.top_cond(17, fm, fv)
        info = e1.state_info()
        assert not info["deferred"] and info["realize_calls"] == 1 and info["listed_launches"] == 0, info
        want = _check(e0, e0.amplitudes(), 17, fixed, "stored %s" % fixed)
        _same(got, want)
        _same(e1.top_cond(17, fm, fv), want)
        assert e1.state_info()["realize_calls"] == 1                      # realised once
        dc.same(e0.amplitudes(), e1.amplitudes())
    finally:
        e0.close()
        e1.close()


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_engine_usable(lib, planted):
    """every QSV_E_BADARG with its message, before the first launch.  Not here: QSV_E_UNSUPPORTED, more than 28 fixed
    bits local to a shard, needs L >= 29 -- an 8 GiB shard, beyond what a quick test holds (the check is the one of
    qsv_sample_cond and qsv_marginals_cond, line for line)."""
    eng, amps = planted.plant("random", lambda: tc.random_state(N, 41))
    eng.reset_stats()
    bad = [
        (0, 0, 0, "k = 0, 1..64"),
        (65, 0, 0, "k = 65, 1..64"),
        (-3, 0, 0, "k = -3"),
        (1, 0b100, 0b110, "fix_val has bits outside fix_mask"),
        (1, 1 << N, 0, "fix_mask has bits at or above qubit %d" % N),
        (64, 1 << 40, 1 << 40, "at or above qubit %d" % N),
    ]
    L = lib.load()
    idx, pp, n = (C.c_uint64 * 64)(), (C.c_double * 64)(), C.c_int(0)
    for k, fm, fv, text in bad:
        assert L.qsv_top_cond(eng._h, k, fm, fv, idx, pp, C.byref(n)) == -1
        assert text.encode() in L.qsv_last_error(), (text, L.qsv_last_error())
        with pytest.raises(ValueError) as e:
            eng.top_cond(k, fm, fv)
        assert text in str(e.value), (text, str(e.value))
    for args in ((None, 1, 0, 0, idx, pp, C.byref(n)), (eng._h, 1, 0, 0, None, pp, C.byref(n)), (eng._h, 1, 0, 0, idx, None, C.byref(n)),
                 (eng._h, 1, 0, 0, idx, pp, None)):
        assert L.qsv_top_cond(*args) == -1 and b"NULL" in L.qsv_last_error()
    assert eng.stats()["kinds"].get("prob", {"launches": 0})["launches"] == 0     # refused before the first launch
    _check(eng, amps, 17, tc.MASKS["mixed"], "after the refusals")


# ---------------------------------------------------------------------------------------------------------------------
# the model level
# ---------------------------------------------------------------------------------------------------------------------
def _p_evidence(cliques, th, evidence):
    from qcmrf_amd import mrf
    n = mrf.num_vertices(cliques)
    p, _ = mrf.gibbs_pmf(cliques, th)
    m, val = mrf._evidence_mask(n, evidence)
    xid = np.arange(p.size)
    return float(p[(xid & m) == val].sum())


@pytest.mark.parametrize("graph", ["chain3", "triangle", "k4"])
@pytest.mark.parametrize("how", ["constructed", "lowered"])
def test_qcmrf_map_states(lib, graph, how):
    from qcmrf_amd import QCMRF, mrf
    from qcmrf_amd.backend import QsvBackend
    cliques, seed, evidence = tc.MODELS[graph]
    th = random_theta(mrf.dimension(cliques), seed=seed)
    qc = QCMRF(cliques, th)
    circuit = None
    if how == "lowered":
        from qcmrf_amd.transpile import transpile
        circuit = transpile(qc, basis_gates=['cx', 'id', 'rz', 'sx', 'x'])
    be = QsvBackend()
    try:
        for k in tc.MODEL_KS:
            for ev in (None, evidence):
                x, p, pc = qc.map_states(be, k=k, evidence=ev, circuit=circuit)
                wx, wp = mrf.map_states(cliques, th, k=k, evidence=ev)
                wpc = mrf.success_probability(cliques, th) * _p_evidence(cliques, th, ev)
                print("QCMRF.map_states %s %s k=%d %s: max p error %.3g, p_condition error %.3g"
                      % (graph, how, k, ev, np.abs(p - wp).max(), abs(pc - wpc)))
                assert x.shape == wx.shape and np.array_equal(x, wx)
                assert np.abs(p - wp).max() < 1e-10
                assert abs(pc - wpc) < 1e-10
    finally:
        be.close()


def test_qcmrf_map_states_keeps_a_deferred_state_deferred(lib):
    from qcmrf_amd import QCMRF, mrf
    from qcmrf_amd.backend import QsvBackend
    cliques, seed, evidence = tc.MODELS["chain8"]                          # 16 qubits: wide enough for the generator to defer its state
    th = random_theta(mrf.dimension(cliques), seed=seed)
    be = QsvBackend(engine_options={"defer_state": 1, "post_select_list": 1})
    try:
        for k, ev in ((1, None), (5, evidence)):
            x, p, pc = QCMRF(cliques, th).map_states(be, k=k, evidence=ev)
            info = be.last_engine.state_info()
            assert info["deferred"] and info["realize_calls"] == 0, info
            wx, wp = mrf.map_states(cliques, th, k=k, evidence=ev)
            assert np.array_equal(x, wx) and np.abs(p - wp).max() < 1e-10
            assert abs(pc - mrf.success_probability(cliques, th) * _p_evidence(cliques, th, ev)) < 1e-10
    finally:
        be.close()
