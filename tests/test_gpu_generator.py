"""k_init_prod, the persistent write-only generator (init x diagonal factors): every tile geometry, class of table
index bit (lane, wave-uniform, register), implied-zero placement and factor-list shape against the numpy engine;
the norm from its tile sums against the k_multi path (init_prod = 0), and sampling from them unchanged by the size
of the persistent grid."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W = 16
TOL = 1e-12
MAXLIST = 10                    # QSV_MULTI_MAXLIST

# the tile on the top bits (init_prod_bit0 -1) of a 16-qubit shard at R = 4, lane map on: lane bits 0..4 and 11,
# wave bits 5 and 6, block bits 7..10, register bits 12..15


def _table(rs, k):
    return np.exp(1j * rs.randn(2 ** k)) * (0.5 + rs.rand(2 ** k))


def _ops(zero, factors, seed):
    from qcmrf_amd import ir
    rs = np.random.RandomState(seed)
    mask = (1 << W) - 1
    for q in zero:
        mask &= ~(1 << q)
    return [ir.op_init(mask)] + [ir.op_diag(qs, _table(rs, len(qs))) for qs in factors]


def _random_factors(zero, n, seed, pool=None, kmax=4):
    rs = np.random.RandomState(seed)
    pool = [q for q in (range(W) if pool is None else pool) if q not in zero]
    out = []
    for _ in range(n):
        k = int(rs.randint(1, min(kmax, len(pool)) + 1))
        out.append([int(q) for q in rs.choice(pool, size=k, replace=False)])
    return out


def _run(ops, devices=1, **opts):
    from qcmrf_amd import _lib, program
    rec, data = program.encode(ops)
    eng = _lib.Engine(W, devices=(0,) * devices)
    for k, v in opts.items():
        eng.set_option(k, v)
    eng.reset_stats()
    eng.exec(rec, data)
    kinds = eng.stats()["kinds"]
    amp = eng.amplitudes()
    norm = eng.norm()
    counts = eng.sample(3000, 11)
    eng.close()
    return amp, norm, counts, kinds


def _check(ops, devices=1, generator=True, **opts):
    from oracle.sharded_numpy import NumpyEngine
    from qcmrf_amd import program
    rec, data = program.encode(ops)
    ref = NumpyEngine(W)
    ref.exec(rec, data)
    want = ref.amplitudes()
    amp, norm, counts, kinds = _run(ops, devices, **opts)
    err = float(np.abs(amp - want).max())
    assert err < TOL, err
    if generator:
        assert kinds.get("init_prod", {}).get("launches", 0) >= 1, kinds
    assert abs(norm - float(np.vdot(want, want).real)) < 1e-12 * norm
    assert (np.abs(want[counts.astype(np.int64)]) > 0).all()
    # one workgroup walking every tile: the same tile sums, so the same norm and the same outcomes for the seed
    amp1, norm1, counts1, _ = _run(ops, devices, **dict(opts, init_prod_grid=1))
    assert np.array_equal(amp1, amp) and norm1 == norm and np.array_equal(counts1, counts)
    # the k_multi path (no generator; tiles of its own, so other outcomes for the seed): the same state and norm
    amp0, norm0, _, _ = _run(ops, devices, **dict(opts, init_prod=0))
    assert float(np.abs(amp0 - want).max()) < TOL and abs(norm - norm0) < 1e-13 * norm
    return kinds


@pytest.mark.parametrize("r", [3, 4, 5, 6])
@pytest.mark.parametrize("bit0", [0, -1, 8])
def test_geometry(r, bit0):
    """every R at the three tile placements (bits 6.., the top bits, a middle offset), a top-bit implied zero"""
    zero = [W - 1]
    _check(_ops(zero, _random_factors(zero, 14, seed=r * 10 + bit0), seed=r), init_prod_r=r, init_prod_bit0=bit0)


@pytest.mark.parametrize("lane_map", [0, 1])
@pytest.mark.parametrize("bit0", [0, -1])
def test_lane_map(lane_map, bit0):
    zero = [W - 1]
    _check(_ops(zero, _random_factors(zero, 12, seed=5 + bit0), seed=lane_map), init_prod_r=4, init_prod_bit0=bit0,
           lane_map=lane_map)


@pytest.mark.parametrize("zq,iz", [
    (15, 1),        # the top register bit: the compile-time implied-zero case
    (13, 1),        # another register bit: zreg at run time
    (5, 1),         # a wave bit of the tile (a thread bit)
    (2, 1),         # a lane bit
    (9, 1),         # a block bit: whole tiles skipped
    (15, 0),        # implied_zeros 0: the full write
    (None, 1),      # no zero qubit
])
def test_implied_zero_placement(zq, iz):
    zero = [] if zq is None else [zq]
    _check(_ops(zero, _random_factors(zero, 16, seed=zq or 0), seed=3), init_prod_r=4, init_prod_bit0=-1,
           implied_zeros=iz)


FACTOR_LISTS = {
    "block_only": [[7, 9], [8], [10, 7, 8], [9, 10]],
    "wave_and_block": [[5, 9], [6, 7, 10], [5, 6]],
    "lane_only": [[0, 3], [11, 4, 1], [2]],
    "mixed": [[0, 7, 5], [11, 9], [3, 6, 10, 1], [4, 8]],
    "single_register": [[12, 0, 9], [13], [14, 5, 11], [12, 7], [13, 2]],
    "multi_register": [[12, 13], [12, 14, 3], [13, 14, 8, 0], [12, 13, 14]],
    "every_list_length": None,          # 1 .. MAXLIST bits, drawn over every class of bit (below)
}


@pytest.mark.parametrize("name", sorted(FACTOR_LISTS))
def test_factor_lists(name):
    zero = [15]
    fl = FACTOR_LISTS[name]
    if fl is None:
        rs = np.random.RandomState(1)
        fl = [[int(q) for q in rs.choice(range(15), size=k, replace=False)] for k in range(1, MAXLIST + 1)]
    _check(_ops(zero, fl, seed=7), init_prod_r=4, init_prod_bit0=-1)


def test_no_factors():
    """an init alone is not a generator pass (k_init); it stays right"""
    _check(_ops([15], [], seed=1), generator=False, init_prod_r=4, init_prod_bit0=-1)


def test_more_factors_than_a_launch_holds():
    """150 factors, pass_max_ops 512: the generator takes the 112 of the first group (factors 64.. use the second lane
    of every wave's descriptors), k_multi the rest"""
    zero = [15]
    kinds = _check(_ops(zero, _random_factors(zero, 150, seed=2, kmax=3), seed=4), init_prod_r=4, init_prod_bit0=-1,
                   pass_max_ops=512)
    assert kinds["init_prod"]["launches"] == 1 and kinds.get("multi", {}).get("launches", 0) >= 1, kinds


def test_tables_at_lds_limit():
    """2556 table entries: two 10-bit tables and one of each length 8..2"""
    zero = [15]
    rs = np.random.RandomState(9)
    fl = [[int(q) for q in rs.choice(range(15), size=k, replace=False)] for k in (10, 10, 8, 7, 6, 5, 4, 3, 2)]
    assert sum(2 ** len(qs) for qs in fl) == 2556
    _check(_ops(zero, fl, seed=8), init_prod_r=4, init_prod_bit0=-1)


@pytest.mark.parametrize("grid", [1, 3, 7])
def test_grid_not_a_divisor(grid):
    """a persistent grid that does not divide the tile count (2^16 / 16 / 256 = 16 tiles)"""
    zero = [15]
    _check(_ops(zero, _random_factors(zero, 12, seed=grid), seed=grid), init_prod_r=4, init_prod_bit0=-1,
           init_prod_grid=grid)


@pytest.mark.parametrize("devices", [1, 2, 4])
@pytest.mark.parametrize("bit0", [0, -1])
def test_virtual_shards(devices, bit0):
    zero = [W - 1]
    _check(_ops(zero, _random_factors(zero, 14, seed=devices), seed=devices), devices=devices, init_prod_bit0=bit0)


@pytest.mark.parametrize("nt", [0, 1])
def test_store_forms(nt):
    zero = [W - 1]
    _check(_ops(zero, _random_factors(zero, 10, seed=nt), seed=nt), init_prod_r=4, init_prod_bit0=-1, init_prod_nt=nt)
