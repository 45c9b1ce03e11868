"""qsv_sample_cond word for word against the exact conditional reference (_post_select_cases.conditional_reference) on
|amplitudes|^2 read from the engine: stored states (contiguous and strided compact blocks, less than a row, one entry,
buffer growth), four virtual shards, implied zeros (never loaded), deferred states (tiles listed, not realised) and the
backend's ``run(..., post_select=...)``.  Every case also holds the returned mass against fsum of the masked p."""
import math

import numpy as np
import pytest

import _deferred_cases as dc
import _post_select_cases as pc
import _sampler_cases as sc
from _sampler_reference import TOL_REL, check_inverse_cdf, exact_index_order, sorted_uniforms, unshuffle
from conftest import random_theta

pytestmark = pytest.mark.gpu

SUM_SLACK = 2.5e-13        # the engine's mass against fsum of the masked p (the bound of _sampler_reference's docstring)
SHOTS = 3000


@pytest.fixture(scope="module")
def lib():
    from qcmrf_amd import _lib
    _lib.load()
    assert _lib.device_count() >= 1
    return _lib


def _mask(fixed):
    return sum(1 << q for q in fixed), sum(int(v) << q for q, v in fixed.items())


def _check(eng, p, fixed, shots, seed, what=None):
    """one conditioned call: the mass, every word (nothing near a boundary), the mask in every word"""
    fm, fv = _mask(fixed)
    words, mass = eng.sample_cond(shots, seed, None, fm, fv)
    assert words.dtype == np.uint64 and len(words) == shots
    pm = np.where(pc.match_of(p.size, fm, fv), p, 0.0)
    want_mass = math.fsum(pm.tolist())
    print("post_select %s: mass %.17g fsum %.17g" % (what or fixed, mass, want_mass))
    assert abs(mass - want_mass) <= SUM_SLACK * want_mass, (what, fixed)
    if shots:
        want, dist, r, _ = pc.conditional_reference(p, fm, fv, seed, shots, total=mass)
        assert int((dist <= TOL_REL * mass).sum()) == 0, (what, fixed, float(dist.min()))
        x = unshuffle(seed, shots, words)
        bad = np.flatnonzero(x != want)
        assert bad.size == 0, (what, fixed, bad.size, bad[:5].tolist(), x[bad[:5]].tolist(), want[bad[:5]].tolist())
        assert ((words & np.uint64(fm)) == np.uint64(fv)).all()
    return words, mass


# ---------------------------------------------------------------------------------------------------------------------
# stored states
# ---------------------------------------------------------------------------------------------------------------------
N = 14
_STATE = {}


def _stored(seed=41):
    if seed not in _STATE:
        v = sc.rand_state(N, seed)
        v.setflags(write=False)
        _STATE[seed] = (v, sc.probs(v))
    return _STATE[seed]


F11 = {q: (q * 5 + 1) % 3 % 2 for q in range(11)}                      # 8 matching entries: bits 11, 12, 13 free
ALL14 = {q: (0b10110011010101 >> q) & 1 for q in range(N)}              # one entry
STORED_CASES = {
    "contiguous_blocks": ({12: 0, 13: 1}, SHOTS, 51),
    "strided": ({0: 1, 3: 0, 5: 1}, SHOTS, 52),
    "mixed": ({2: 1, 7: 0, 13: 1}, SHOTS, 53),
    "less_than_a_row": (F11, SHOTS, 54),
    "one_entry": (ALL14, SHOTS, 55),
    "70000_shots": ({12: 1, 13: 0}, 70000, 56),
}


@pytest.mark.parametrize("name", sorted(STORED_CASES))
def test_stored_state(lib, name):
    fixed, shots, seed = STORED_CASES[name]
    v, p = _stored()
    with lib.Engine(N) as eng:
        eng.set_amplitudes(0, v)
        eng.reset_stats()
        words, mass = _check(eng, p, fixed, shots, seed, name)
        k = eng.stats()["kinds"]["prob"]
        assert k["launches"] == 1 and k["bytes"] == 16.0 * (1 << (N - len(fixed)))     # 2^-f of the shard is read
        if name == "one_entry":
            assert (words == np.uint64(_mask(fixed)[1])).all()
        # not cached: a second call repeats the pass, and gives the same words
        again, mass2 = eng.sample_cond(shots, seed, None, *_mask(fixed))
        assert np.array_equal(again, words) and mass2 == mass and eng.stats()["kinds"]["prob"]["launches"] == 2


def test_mask_zero_is_sample_word_for_word(lib):
    v, p = _stored()
    with lib.Engine(N) as eng:
        eng.set_amplitudes(0, v)
        words, mass = eng.sample_cond(SHOTS, 57)
        assert np.array_equal(words, eng.sample(SHOTS, 57)) and mass == eng.norm()
        meas = [3, -1, 13, 0]
        w2, _ = eng.sample_cond(SHOTS, 58, meas)
        assert np.array_equal(w2, eng.sample(SHOTS, 58, meas))
        none, mass0 = eng.sample_cond(0, 1, None, 1 << 13, 0)
        assert len(none) == 0 and 0 < mass0 < mass


def test_measured_bits_are_remapped(lib):
    v, p = _stored()
    meas = [13, -1, 2, 7, 0]
    fm, fv = _mask({2: 1, 7: 0, 13: 1})
    with lib.Engine(N) as eng:
        eng.set_amplitudes(0, v)
        full, _ = eng.sample_cond(SHOTS, 59, None, fm, fv)
        got, _ = eng.sample_cond(SHOTS, 59, meas, fm, fv)
    want = np.zeros_like(full)
    for j, q in enumerate(meas):
        if q >= 0:
            want |= ((full >> np.uint64(q)) & np.uint64(1)) << np.uint64(j)
    assert np.array_equal(got, want)


def test_bad_arguments(lib):
    v, p = _stored()
    with lib.Engine(N) as eng:
        eng.set_amplitudes(0, v)
        with pytest.raises(ValueError):
            eng.sample_cond(10, 1, None, 0b100, 0b110)            # a value bit outside the mask
        with pytest.raises(ValueError):
            eng.sample_cond(10, 1, None, 1 << N, 0)               # a mask bit at W


def test_zero_probability_is_refused_and_leaves_the_engine_usable(lib):
    v = np.array(sc.rand_state(N, 43))
    v[1 << 13:] = 0
    v /= np.linalg.norm(v)
    p = sc.probs(v)
    with lib.Engine(N) as eng:
        eng.set_amplitudes(0, v)
        with pytest.raises(ValueError, match="zero probability"):
            eng.sample_cond(SHOTS, 60, None, 1 << 13, 1 << 13)
        none, mass = eng.sample_cond(0, 60, None, 1 << 13, 1 << 13)
        assert mass == 0.0
        total = eng.norm()
        words = eng.sample(SHOTS, 61)
        r = sorted_uniforms(61, SHOTS, total)
        want, dist = exact_index_order(p, r)
        assert int((dist <= TOL_REL * total).sum()) == 0
        assert np.array_equal(unshuffle(61, SHOTS, words), want)
        _check(eng, p, {13: 0, 4: 1}, SHOTS, 62)


# ---------------------------------------------------------------------------------------------------------------------
# four virtual shards (L = 12)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fixed", [{13: 1}, {12: 0, 4: 1}, {13: 0, 12: 1, 11: 1}], ids=["13", "12_4", "13_12_11"])
def test_four_virtual_shards(lib, fixed):
    v, p = _stored(42)
    with lib.Engine(N, devices=(0,) * 4) as eng:
        eng.set_amplitudes(0, v)
        _check(eng, p, fixed, SHOTS, 63 + len(fixed))


# ---------------------------------------------------------------------------------------------------------------------
# implied zeros: the zero half of the state is undefined memory, never loaded
# ---------------------------------------------------------------------------------------------------------------------
def test_implied_zeros_are_not_read(lib):
    W, P, _, _, _ = sc.TILE_PROGRAMS["generator_P1"]
    rec, data, want = sc.tile_reference("generator_P1")
    zero = 15                                                              # generator_only(1): the top qubit stays |0>
    with lib.Engine(W) as eng:
        eng.set_option("implied_zeros", 1)
        eng.set_option("defer_state", 0)
        eng.set_amplitudes(0, np.full(1 << W, 1.0 + 1.0j))               # whatever the program does not write is not zero
        eng.exec(rec, data)
        got = eng.amplitudes()
        assert np.abs(got - want).max() < 1e-12
        assert not got[1 << zero:].any()
        p = sc.probs(got)
        _check(eng, p, {zero: 0, 3: 1, 9: 0}, SHOTS, 71)
        _check(eng, p, {2: 1, 8: 0}, SHOTS, 72)                           # the zero qubit free: half of the sub-cube is implied
        _check(eng, p, {13: 1, 14: 0}, SHOTS, 73)                         # contiguous compact blocks, every other one implied
        with pytest.raises(ValueError, match="zero probability"):
            eng.sample_cond(SHOTS, 74, None, 1 << zero, 1 << zero)
        assert not eng.state_info()["deferred"]


# ---------------------------------------------------------------------------------------------------------------------
# deferred states, W = 16: lane bits 0..4 and 11, wave bits 5 and 6, block bits 7..10, register bits 12..15
# ---------------------------------------------------------------------------------------------------------------------
GEOMETRY = {"init_prod_r": 4, "init_prod_bit0": -1}
LISTED = [{7: 1}, {8: 0}, {9: 1}, {10: 0}, {8: 1, 10: 1}, {9: 0, 3: 1}, {7: 1, 5: 0}, {10: 1, 14: 1}]


def _start(ops, defer, w=dc.W, devices=1, **opts):
    """_deferred_cases.start with the memory pre-filled before the program runs"""
    from qcmrf_amd import _lib, program
    rec, data = program.encode(ops)
    eng = _lib.Engine(w, devices=(0,) * devices)
    for k, v in opts.items():
        eng.set_option(k, v)
    eng.set_option("defer_state", defer)
    eng.set_amplitudes(0, np.full(1 << w, 1.0 + 1.0j))
    eng.reset_stats()
    eng.exec(rec, data)
    return eng


def _pair(ops, devices=1, **opts):
    e0 = _start(ops, 0, devices=devices, **opts)
    e1 = _start(ops, 1, devices=devices, **opts)
    assert e1.state_info()["deferred"] and not e0.state_info()["deferred"]
    return e0, e1, sc.probs(e0.amplitudes())


def _both(e0, e1, p, fixed, seed):
    """the same call on the written and on the deferred engine: equal words and masses, and the reference's"""
    w0, m0 = _check(e0, p, fixed, SHOTS, seed)
    fm, fv = _mask(fixed)
    w1, m1 = e1.sample_cond(SHOTS, seed, None, fm, fv)
    assert np.array_equal(w0, w1) and m0 == m1, fixed


@pytest.mark.parametrize("group", [-1, 0])
def test_deferred_state_lists_the_tiles(lib, group):
    ops = dc.default_ops(seed=7)
    e0, e1, p = _pair(ops, post_select_list=1, init_prod_group=group, **GEOMETRY)
    try:
        for i, fixed in enumerate(LISTED):
            before = e1.state_info()
            _both(e0, e1, p, fixed, 80 + i)
            after = e1.state_info()
            assert after["deferred"] and after["realize_calls"] == before["realize_calls"] == 0, (fixed, after)
            assert after["listed_launches"] == before["listed_launches"] + 1, (fixed, after)
        # the deferred engine is still a sampler of the whole state, and still writes the same state
        total = e1.norm()
        words = e1.sample(SHOTS, 90)
        assert e1.state_info()["deferred"]
        r = sorted_uniforms(90, SHOTS, total)
        assert check_inverse_cdf(p, r, unshuffle(90, SHOTS, words), TOL_REL * total, total) == []
        dc.same(e0.amplitudes(), e1.amplitudes())
        assert e1.state_info()["realize_calls"] == 1
    finally:
        e0.close()
        e1.close()


@pytest.mark.parametrize("option,fixed,listed", [(1, {3: 1}, False), (0, {7: 1}, False), (0, {7: 0, 8: 1, 9: 0, 10: 1}, False),
                                                 (-1, {7: 0, 8: 1, 9: 1, 10: 0}, True), (-1, {7: 1}, False), (-1, {3: 0}, False)])
def test_deferred_state_path_by_option(lib, option, fixed, listed):
    """no block bit fixed: always realised; post_select_list 0: always realised; -1: listed up to 1 tile in 16"""
    e0, e1, p = _pair(dc.default_ops(seed=8), post_select_list=option, **GEOMETRY)
    try:
        _both(e0, e1, p, fixed, 91)
        info = e1.state_info()
        if listed:
            assert info["deferred"] and info["realize_calls"] == 0 and info["listed_launches"] == 1, info
        else:
            assert not info["deferred"] and info["realize_calls"] == 1 and info["listed_launches"] == 0, info
        dc.same(e0.amplitudes(), e1.amplitudes())
    finally:
        e0.close()
        e1.close()


def test_deferred_state_two_shards(lib):
    """L = 15: register bits 11..14, block bits 8..10 on either shard; one listed launch per shard that matches"""
    e0, e1, p = _pair(dc.default_ops(seed=9), devices=2, post_select_list=1, **GEOMETRY)
    try:
        _both(e0, e1, p, {9: 1, 2: 0}, 92)
        info = e1.state_info()
        assert info["deferred"] and info["realize_calls"] == 0 and info["listed_launches"] == 2, info
        _both(e0, e1, p, {15: 0, 10: 0}, 93)                              # a shard bit: shard 1 is skipped
        info = e1.state_info()
        assert info["deferred"] and info["realize_calls"] == 0 and info["listed_launches"] == 3, info
        dc.same(e0.amplitudes(), e1.amplitudes())
    finally:
        e0.close()
        e1.close()


# ---------------------------------------------------------------------------------------------------------------------
# through run()
# ---------------------------------------------------------------------------------------------------------------------
RUN_OPTIONS = {"default": {}, "no_fold": {"fold_fresh": False}, "gate_by_gate": {"fusion": 0}, "four_shards": {"devices": (0,) * 4},
               "deferred_listed": {"engine_options": {"defer_state": 1, "post_select_list": 1}}, "lowered": {}}


CHAIN4, TRIANGLES = [[0, 1], [1, 2], [2, 3]], [[0, 1, 2], [2, 3, 4]]
CHAIN8 = [[i, i + 1] for i in range(7)]                # 16 qubits: wide enough for the generator to defer its state
RUN_CASES = [(name, "chain4") for name in sorted(RUN_OPTIONS)] + [(name, "triangles") for name in sorted(RUN_OPTIONS) if name != "lowered"] + \
            [("deferred_listed", "chain8")]


@pytest.mark.parametrize("name,graph", RUN_CASES)      # (the lowered circuit runs once)
def test_through_run(lib, name, graph):
    from qcmrf_amd import QCMRF, mrf
    from qcmrf_amd.backend import QsvBackend
    from qcmrf_amd.qcmrf import extract_probs
    cliques = {"chain4": CHAIN4, "triangles": TRIANGLES, "chain8": CHAIN8}[graph]
    n, m = mrf.num_vertices(cliques), len(cliques)
    W = n + m + 1
    th = random_theta(mrf.dimension(cliques))
    qc = QCMRF(cliques, th)
    post = qc.post_selection()
    circ = qc
    if name == "lowered":
        from qcmrf_amd.transpile import transpile
        circ = transpile(qc, basis_gates=['cx', 'id', 'rz', 'sx', 'x'])
    shots, seed = 4096, 97
    be = QsvBackend(**RUN_OPTIONS[name])
    try:
        res = be.run(circ, shots=shots, seed_simulator=seed, post_select=post).result()
        counts, md = res.get_counts(), res.metadata(0)
        assert md["post_select"] == post and md["post_select_path"] in ("stored", "listed", "realized")
        print("post_select run %s: path %s probability %.17g" % (name, md["post_select_path"], md["post_select_probability"]))
        if graph == "chain8":                                             # the generator deferred the state: not read as stored
            assert md["post_select_path"] in ("listed", "realized"), md["post_select_path"]
        lay = md["layout"]
        p = sc.probs(be.last_engine.amplitudes())
        logical = sc.probs(be.statevector())
    finally:
        be.close()
    fm = sum(1 << lay[c] for c in post)                                   # classical bit c <- qubit c in a QCMRF circuit
    want, dist, r, mass = pc.conditional_reference(p, fm, 0, seed, shots)
    assert int((dist <= TOL_REL * mass).sum()) == 0
    vals = np.zeros_like(want)
    for c in range(W):
        if c != n:                                                        # the AND scratch qubit is not measured
            vals |= ((want >> np.uint64(lay[c])) & np.uint64(1)) << np.uint64(c)
    uv, uc = np.unique(vals, return_counts=True)
    assert counts == {format(int(v), "0%db" % W): int(c) for v, c in zip(uv, uc)}
    assert all(len(k) == W and k[:m] == "0" * m for k in counts)
    assert abs(md["post_select_probability"] - mrf.success_probability(cliques, th)) < 1e-12
    # the exact conditional pmf: ancillas 0, the scratch qubit summed over
    g = np.arange(1 << W)
    sel = (g >> (n + 1)) == 0
    pmf = np.bincount(g[sel] & ((1 << n) - 1), weights=logical[sel], minlength=1 << n)
    assert np.abs(pmf / pmf.sum() - mrf.gibbs_pmf(cliques, th)[0]).max() < 1e-10
    P, delta = extract_probs(counts, n, m + 1)
    assert delta == 1.0
