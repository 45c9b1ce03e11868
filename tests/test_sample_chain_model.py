"""The device walk over the super sums (option sample_chain, k_walk_super / k_walk_shots) against the host walk of
qsv_sample, both restated in numpy doubles (tests/_sample_chain_model.py): the same (block, residual) for every shot,
the same total bit for bit, and the two mistakes a device walk could make are seen by a case here."""
import numpy as np
import pytest

import _sample_chain_model as m

SIZES = [1, 2, 64, 128, 4096]
SHAPES = ["random", "leading", "trailing", "interior", "one"]
CASES = [(n, sh) for n in SIZES for sh in SHAPES if n > 1 or sh in ("random", "one")]   # one entry has no zeros beside it


def _sums(n, seed, shape="random"):
    rs = np.random.RandomState(seed)
    bs = rs.rand(n) * np.exp(4.0 * rs.randn(n))         # many magnitudes: the sequential and pairwise sums differ
    if shape == "leading":
        bs[:max(1, n // 3)] = 0.0
    elif shape == "trailing":
        bs[n - max(1, n // 3):] = 0.0
    elif shape == "interior":
        bs[rs.rand(n) < 0.4] = 0.0
        bs[n // 2] = 0.0
    elif shape == "one":
        k = int(rs.randint(n))
        v = bs[k]
        bs[:] = 0.0
        bs[k] = v
    if not (bs > 0).any():
        bs[0] = 1.0
    return bs


def _bits(pairs):
    return [(b, np.float64(r).tobytes()) for b, r in pairs]


def _both(bs, r):
    host, dev = m.host_walk(bs, r), m.device_walk(bs, r)
    assert _bits(host) == _bits(dev)
    return host


@pytest.mark.parametrize("n", SIZES)
def test_total_has_pairwise_sums_association(n):
    for seed in range(4):
        bs = _sums(n, seed)
        assert np.float64(m.device_total(bs)).tobytes() == np.float64(m.pairwise_sum(bs)).tobytes()
    if n >= 128:                                        # and the association matters at these sizes
        assert any(m.pairwise_sum(_sums(n, s)) != float(np.cumsum(_sums(n, s))[-1]) for s in range(8))


@pytest.mark.parametrize("n,shape", CASES)
def test_same_block_and_residual(n, shape):
    for seed in range(3):
        bs = _sums(n, 10 * seed + 1, shape)
        total = m.pairwise_sum(bs)
        for shots in (1, 2, 700):
            raw, run = m.spacings(shots, seed + shots)
            got = _both(bs, m.uniforms(total, raw, run))
            assert all(0 <= b < n and r >= 0.0 for b, r in got)
            assert [b for b, _ in got] == sorted(b for b, _ in got)


@pytest.mark.parametrize("n,shape", CASES)
def test_uniforms_on_the_edges(n, shape):
    """positions equal to a prefix value (the walk must step past it), just below one, 0 and nextafter(total, 0)"""
    bs = _sums(n, 5, shape)
    total = m.pairwise_sum(bs)
    cap = float(np.nextafter(total, 0.0))
    pre = [float(v) for v in np.cumsum(bs)]             # numpy's cumsum adds one after the other
    pick = sorted(set(pre[::max(1, n // 50)] + pre[-2:]))
    r = sorted(min(v, cap) for v in [0.0, cap] + pick + [float(np.nextafter(v, 0.0)) for v in pick if v > 0])
    got = _both(bs, r)
    assert max(b for b, _ in got) <= m.last_nonzero(bs)


def test_a_missing_clamp_is_seen():
    """trailing zeros and a position at the end of the mass: the host stays in the last populated entry"""
    seen = 0
    for n in SIZES[1:]:
        bs = _sums(n, 5, "trailing")
        r = [float(np.cumsum(bs)[-1])]
        host = m.host_walk(bs, r)
        assert _bits(host) == _bits(m.device_walk(bs, r))
        seen += _bits(host) != _bits(m.device_walk(bs, r, clamp=False))
    assert seen == len(SIZES) - 1


def test_a_wrong_comparison_is_seen():
    """a position equal to an interior prefix value belongs to the next entry: r <= P[b + 1] keeps it in b"""
    seen = 0
    for n in SIZES[1:]:
        bs = _sums(n, 7)
        r = [float(np.cumsum(bs)[n // 2 - 1])]
        host = m.host_walk(bs, r)
        assert host[0][0] == n // 2 and _bits(host) == _bits(m.device_walk(bs, r))
        seen += _bits(host) != _bits(m.device_walk(bs, r, strict=False))
    assert seen == len(SIZES) - 1
