"""Host checks of the exact sampler reference (_sampler_reference.py): the generator against the value the C++
standard fixes, the shuffle round trip, the layout-independent contract accepted for every walk order and REJECTED for
each way the sampler could be subtly wrong, and -- for the GPU cases that demand word equality -- that no uniform of
theirs lies within the tolerance of a prefix boundary."""
import math

import numpy as np
import pytest

import _sampler_cases as sc
from _sampler_reference import (MT64, RULES, TOL_REL, check_inverse_cdf, exact_index_order, model_sampler, rules_of,
                                shuffle_swaps, sorted_uniforms, unshuffle)


def test_mt64_known_value():
    """[rand.predef]: the 10000th consecutive invocation of a default-constructed mt19937_64 (seed 5489)"""
    rng = MT64(5489)
    out = rng.draw(10000)
    assert int(out[-1]) == 9981545732273789042
    one = MT64(5489)                                          # call by call and in uneven chunks: the same stream
    assert [one() for _ in range(5)] == [int(v) for v in out[:5]]
    chunks = MT64(5489)
    assert np.array_equal(np.concatenate([chunks.draw(k) for k in (1, 311, 313, 0, 624, 8751)]), out)


def test_sorted_uniforms_are_sorted_scaled_and_clamped():
    for total in (1.0, 3.7, 2.0 ** -40):
        r = sorted_uniforms(77, 5000, total)
        assert r.dtype == np.float64 and len(r) == 5000
        assert (np.diff(r) >= 0).all() and r[0] > 0 and r[-1] < total
    assert len(sorted_uniforms(77, 0, 1.0)) == 0
    # the generator is left where the shuffle picks it up: shots + 1 draws in
    rng = MT64(9)
    sorted_uniforms(9, 10, 1.0, rng=rng)
    ref = MT64(9)
    ref.draw(11)
    assert rng() == ref()


@pytest.mark.parametrize("shots", [1, 2, 3, 1000, 8193])
def test_unshuffle_round_trip(shots):
    """a forward Fisher-Yates written here from the sampler's description, one generator call per step"""
    seed = 1000 + shots
    rng = MT64(seed)
    for _ in range(shots + 1):
        rng()
    words = [7 * s + 3 for s in range(shots)]
    fwd = list(words)
    for s in range(shots - 1, 0, -1):
        k = rng() % (s + 1)
        fwd[s], fwd[k] = fwd[k], fwd[s]
    back = unshuffle(seed, shots, np.array(fwd, dtype=np.uint64))
    assert back.dtype == np.uint64 and back.tolist() == words
    if shots > 100:
        assert fwd != words
    s, k = shuffle_swaps(seed, shots)
    assert len(s) == max(shots - 1, 0) and (k <= s).all()


# ---------------------------------------------------------------------------------------------------------------------
# the contract: accepted for every order of the walk
# ---------------------------------------------------------------------------------------------------------------------
N, SHOTS = 1 << 14, 70000


def _state(kind, seed=3):
    rs = np.random.RandomState(seed)
    p = rs.randn(N) ** 2 + rs.randn(N) ** 2
    if kind == "half_empty":
        p[(np.arange(N) & 0b1000) != 0] = 0
    elif kind == "empty_blocks":
        p[:4096] = 0
        p[8192:12288] = 0
    elif kind == "single":
        p[:] = 0
        p[5000] = 1.0
    p /= p.sum()
    if kind == "unnormalised":
        p *= 3.7
    return p


def _orders(seed=5):
    rs = np.random.RandomState(seed)
    tile = np.arange(N).reshape(-1, 32, 16).transpose(0, 2, 1).reshape(-1) ^ 0x2a40     # strided tiles through an X frame
    return {"index": np.arange(N), "perm_a": rs.permutation(N), "perm_b": rs.permutation(N), "tiles": tile}


@pytest.mark.parametrize("kind", ["full", "half_empty", "empty_blocks", "single", "unnormalised"])
def test_contract_holds_for_any_walk_order(kind):
    p = _state(kind)
    total = math.fsum(p.tolist())
    assert abs(total - (3.7 if kind == "unnormalised" else 1.0)) < 1e-12
    r = sorted_uniforms(11, SHOTS, total)
    for name, order in _orders().items():
        x = model_sampler(p, order, r)
        assert check_inverse_cdf(p, r, x, TOL_REL * total) == [], (kind, name)
    idx, dist = exact_index_order(p, r)
    assert np.array_equal(idx, model_sampler(p, np.arange(N), r))
    assert (dist > 0).all()
    if kind == "single":
        assert (idx == 5000).all() and np.isinf(dist).all()


def test_contract_through_the_shuffle():
    """words as the sampler returns them (shuffled): unshuffle, then check"""
    p = _state("half_empty")
    seed, shots = 21, 20000
    r = sorted_uniforms(seed, shots, 1.0)
    x = model_sampler(p, _orders()["tiles"], r)
    s, k = shuffle_swaps(seed, shots)
    out = x.copy()
    for a, b in zip(s.tolist(), k.tolist()):
        out[a], out[b] = out[b], out[a]
    assert not np.array_equal(out, x)
    assert check_inverse_cdf(p, r, unshuffle(seed, shots, out), TOL_REL) == []


def test_exact_index_order_small():
    p = np.array([0.0, 0.25, 0.0, 0.5, 0.25, 0.0])
    r = np.array([0.0, 0.1, 0.25, 0.3, 0.75, 0.875, np.nextafter(1.0, 0.0)])
    idx, dist = exact_index_order(p, r)
    assert idx.tolist() == [1, 1, 3, 3, 4, 4, 4]
    assert np.allclose(dist, [0.25, 0.15, 0.0, 0.05, 0.0, 0.125, 0.25])
    assert check_inverse_cdf(p, r, idx, TOL_REL) == []


# ---------------------------------------------------------------------------------------------------------------------
# ... and rejected for each error the sampler could make (the reduced chi-square of these stays inside 1 +- 0.05)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def base():
    p = _state("half_empty")
    r = sorted_uniforms(11, SHOTS, 1.0)
    order = np.arange(N)
    x = model_sampler(p, order, r)
    assert check_inverse_cdf(p, r, x, TOL_REL) == []
    return p, r, x


def _fires(p, r, x, expected):
    got = rules_of(check_inverse_cdf(p, r, x, TOL_REL))
    assert set(got) <= set(RULES)
    assert set(expected) & set(got), (expected, got)
    return got


def test_mutation_shots_moved_to_the_previous_support_index(base):
    p, r, x = base
    rs = np.random.RandomState(1)
    sup = np.flatnonzero(p > 0)
    pos = np.searchsorted(sup, x.astype(np.int64))
    pick = rs.choice(np.flatnonzero(pos > 0), size=SHOTS // 200, replace=False)       # 0.5 % of the shots
    y = x.copy()
    y[pick] = sup[pos[pick] - 1]
    cnt_x, cnt_y = np.bincount(x.astype(np.int64), minlength=N), np.bincount(y.astype(np.int64), minlength=N)
    sel = p * SHOTS > 3
    chi = lambda c: ((c[sel] - p[sel] * SHOTS) ** 2 / (p[sel] * SHOTS)).sum() / (sel.sum() - 1)
    assert abs(chi(cnt_y) - chi(cnt_x)) < 0.05               # what the statistical tests see: nothing
    _fires(p, r, y, ["runs"])


def test_mutation_bit_0_flipped(base):
    p, r, x = base
    rs = np.random.RandomState(2)
    pick = rs.choice(SHOTS, size=SHOTS // 50, replace=False)                          # 2 %
    y = x.copy()
    y[pick] ^= np.uint64(1)
    assert (p[y.astype(np.int64)] > 0).all()                # bit 0 is populated on either side: support cannot see it
    _fires(p, r, y, ["runs"])


def test_mutation_uniforms_scaled(base):
    p, r, x = base
    y = model_sampler(p, np.arange(N), r * 0.97)
    got = _fires(p, r, y, ["suffix"])
    assert "runs" not in got and "support" not in got         # a perfectly formed walk, of the wrong uniforms


def test_mutation_one_index_skipped_in_every_4096(base):
    p, r, x = base
    q = p.copy()
    skipped = np.arange(17, N, 4096)
    assert (p[skipped] > 0).all()
    q[skipped] = 0                                             # the walk steps over them; the mass piles up at the end
    y = model_sampler(q, np.arange(N), r)
    _fires(p, r, y, ["upper"])


def test_mutation_greater_or_equal_at_a_boundary_hit_exactly():
    """``>=`` for ``>`` differs only where a uniform equals a prefix sum, and then by one support index whose interval
    the uniform touches: inside the contract for any tol >= 0 (as is every rounding difference), except where the
    index so chosen is empty -- rule ``support``.  The word-exact comparison sees every such shot: the reference
    reports distance 0 there, which is why the GPU cases first show that no uniform of theirs is near a boundary."""
    p = np.array([0.0, 0.25, 0.0, 0.5, 0.25, 0.0])               # dyadic: every prefix sum is exact
    r = np.array([0.0, 0.125, 0.25, 0.5, 0.75])
    cum = np.cumsum(p)
    good = np.searchsorted(cum, r, side="right")
    bad = np.searchsorted(cum, r, side="left")                  # first index with cum >= r
    want, dist = exact_index_order(p, r)
    assert np.array_equal(good, want.astype(np.int64))
    assert check_inverse_cdf(p, r, good, TOL_REL) == []
    assert bad.tolist() == [0, 1, 1, 3, 3]
    differs = bad != good
    assert differs.sum() == 3 and (dist[differs[1:].nonzero()[0] + 1] == 0).all()   # exactly the shots at distance 0
    assert rules_of(check_inverse_cdf(p, r, bad, TOL_REL)) == ["support"]


def test_mutation_shuffle_undone_with_the_wrong_seed(base):
    p, r, x = base
    s, k = shuffle_swaps(11, SHOTS)
    out = x.copy().tolist()
    for a, b in zip(s.tolist(), k.tolist()):
        out[a], out[b] = out[b], out[a]
    out = np.array(out, dtype=np.uint64)
    assert np.array_equal(unshuffle(11, SHOTS, out), x)
    _fires(p, r, unshuffle(12, SHOTS, out), ["runs"])


def test_mutation_two_runs_swapped(base):
    p, r, x = base
    xi = x.astype(np.int64)
    ids, first, counts = np.unique(xi, return_index=True, return_counts=True)
    big = ids[np.argmax(p[ids])]
    far = ids[np.abs(first - first[ids == big][0]) > SHOTS // 4]
    small = far[np.argmin(p[far])]
    y = x.copy()
    y[xi == big] = small
    y[xi == small] = big
    got = _fires(p, r, y, ["upper", "lower", "prefix", "suffix"])
    assert "runs" not in got and "support" not in got         # every index still one run, all inside the support


# ---------------------------------------------------------------------------------------------------------------------
# the GPU cases that demand every word: none of their uniforms is near a prefix boundary
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(sc.INDEX_CASES))
def test_no_shot_near_a_boundary(name):
    """total is fsum(p) here and the engine's own block-sum total on the GPU: they differ by rounding (below
    2.5e-13 of the total, see the reference's docstring), and so do the uniforms scaled by them; counting inside
    2 * tol leaves that room."""
    n, P, steps = sc.INDEX_CASES[name]
    for state, calls in steps():
        assert state.size == 2 ** n
        p = sc.probs(state)
        total = math.fsum(p.tolist())
        tol = TOL_REL * total
        for shots, seed in calls:
            r = sorted_uniforms(seed, shots, total)
            idx, dist = exact_index_order(p, r)
            assert int((dist <= 2 * tol).sum()) == 0, (name, shots, seed, float(dist.min()))
            assert check_inverse_cdf(p, r, idx, tol, total) == []


@pytest.mark.parametrize("name", sorted(sc.TILE_PROGRAMS))
def test_no_shot_near_a_boundary_of_the_tile_programs(name):
    """the programs of the tile-order GPU cases, run here by the numpy engine: with fused_sums = 0 the GPU test demands
    every word, and asserts this margin again on the amplitudes it reads back (they differ from these by rounding)"""
    W, P, _, shots, seed = sc.TILE_PROGRAMS[name]
    p = sc.probs(sc.tile_reference(name)[2])
    total = math.fsum(p.tolist())
    r = sorted_uniforms(seed, shots, total)
    idx, dist = exact_index_order(p, r)
    assert int((dist <= 10 * TOL_REL * total).sum()) == 0, (name, float(dist.min()))
    assert check_inverse_cdf(p, r, idx, TOL_REL * total, total) == []
