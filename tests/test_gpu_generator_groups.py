"""k_init_prod with tile groups (option init_prod_group): a workgroup takes 2^B tiles that differ only in B block bits
and forms what they share once.  Every case runs against the numpy engine; a one-workgroup grid gives the same
amplitudes, norm and outcomes; groups off (init_prod_group 0) gives the same state to the last bits."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-12

# W = 16, R = 4 on the top bits (init_prod_bit0 -1): lane bits 0..4 and 11, wave bits 5 and 6, block bits 7..10 (the
# four tile-index bits), register bits 12..15.  init_prod_group 4 makes every block bit that is not a zero qubit a
# group bit.
BLOCK = [7, 8, 9, 10]


def _table(rs, k):
    return np.exp(1j * rs.randn(2 ** k)) * (0.5 + rs.rand(2 ** k))


def _ops(W, zero, factors, seed):
    from qcmrf_amd import ir
    rs = np.random.RandomState(seed)
    mask = (1 << W) - 1
    for q in zero:
        mask &= ~(1 << q)
    return [ir.op_init(mask)] + [ir.op_diag(qs, _table(rs, len(qs))) for qs in factors]


def _random_factors(W, zero, n, seed, kmax=4):
    rs = np.random.RandomState(seed)
    pool = [q for q in range(W) if q not in zero]
    out = []
    for _ in range(n):
        k = int(rs.randint(1, min(kmax, len(pool)) + 1))
        out.append([int(q) for q in rs.choice(pool, size=k, replace=False)])
    return out


def _run(W, ops, devices=1, **opts):
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


def _check(ops, W=16, devices=1, **opts):
    from oracle.sharded_numpy import NumpyEngine
    from qcmrf_amd import program
    rec, data = program.encode(ops)
    ref = NumpyEngine(W)
    ref.exec(rec, data)
    want = ref.amplitudes()
    amp, norm, counts, kinds = _run(W, ops, devices, **opts)
    assert kinds.get("init_prod", {}).get("launches", 0) >= 1, kinds
    assert float(np.abs(amp - want).max()) < TOL
    assert abs(norm - float(np.vdot(want, want).real)) < 1e-12 * norm
    assert (np.abs(want[counts.astype(np.int64)]) > 0).all()
    # one workgroup walking every group: the same products and tile sums
    amp1, norm1, counts1, _ = _run(W, ops, devices, **dict(opts, init_prod_grid=1))
    assert np.array_equal(amp1, amp) and norm1 == norm and np.array_equal(counts1, counts)
    # groups off: the products in another order
    amp0, norm0, _, _ = _run(W, ops, devices, **dict(opts, init_prod_group=0))
    assert float(np.abs(amp0 - amp).max()) <= 1e-13 * float(np.abs(amp0).max())
    assert abs(norm0 - norm) <= 1e-13 * norm
    return amp, norm, counts


@pytest.mark.parametrize("bit0", [0, -1, 8])
@pytest.mark.parametrize("r", [3, 4, 5, 6])
@pytest.mark.parametrize("b", [0, 1, 2, 3, 4])
def test_group_bits(b, r, bit0):
    """every forced B (fewer where the tile index has fewer bits) at every R and tile placement"""
    zero = [15]
    _check(_ops(16, zero, _random_factors(16, zero, 14, seed=r * 10 + b), seed=r + b), init_prod_r=r,
           init_prod_bit0=bit0, init_prod_group=b)


FACTOR_LISTS = {
    "single_group_bit": [[7], [8, 0], [2, 5]],
    "two_group_bits": [[7, 9], [8, 10, 3], [1, 12]],
    "every_group_bit": [[7, 8, 9, 10], [0, 13], [6]],
    "group_and_register": [[7, 12], [9, 13, 14], [8, 10, 12, 13], [3]],
    "group_and_lane": [[8, 3], [10, 11], [7, 0, 1]],
    "group_and_wave": [[7, 5], [9, 6], [8, 10, 5, 6]],
    "several_on_one_group_bit": [[7], [7, 1], [7, 5, 12], [7, 9]],
}


@pytest.mark.parametrize("b", [4, -1])
@pytest.mark.parametrize("name", sorted(FACTOR_LISTS))
def test_factors_around_group_bits(name, b):
    _check(_ops(16, [15], FACTOR_LISTS[name], seed=3), init_prod_r=4, init_prod_bit0=-1, init_prod_group=b)


@pytest.mark.parametrize("b", [4, -1])
def test_128_factors(b):
    """150 factors, pass_max_ops 512: the generator takes the first group's (factors 64.. on the second descriptor
    lane), k_multi the rest"""
    zero = [15]
    _check(_ops(16, zero, _random_factors(16, zero, 150, seed=2, kmax=3), seed=4), init_prod_r=4, init_prod_bit0=-1,
           pass_max_ops=512, init_prod_group=b)


@pytest.mark.parametrize("b", [4, -1])
def test_tables_at_lds_limit(b):
    """2556 table entries: two 10-bit tables and one of each length 8..2"""
    rs = np.random.RandomState(9)
    fl = [[int(q) for q in rs.choice(range(15), size=k, replace=False)] for k in (10, 10, 8, 7, 6, 5, 4, 3, 2)]
    assert sum(2 ** len(qs) for qs in fl) == 2556
    _check(_ops(16, [15], fl, seed=8), init_prod_r=4, init_prod_bit0=-1, init_prod_group=b)


@pytest.mark.parametrize("b", [4, 3, -1])
@pytest.mark.parametrize("zq", [9, 7])
def test_zero_qubit_on_a_block_bit(zq, b):
    """a provably-zero qubit on a block bit is never a group bit: its tiles are implied zero with sum 0, and implied
    zeros on and off give the same amplitudes, norm and outcomes"""
    zero = [zq]
    # the zero qubit is the block bit no factor touches: the rule would pick it first were it allowed
    fl = [[q for q in qs if q != zq] or [0] for qs in _random_factors(16, zero, 16, seed=zq)]
    ops = _ops(16, zero, fl, seed=5)
    amp, norm, counts = _check(ops, init_prod_r=4, init_prod_bit0=-1, init_prod_group=b)
    amp0, norm0, counts0, kinds = _run(16, ops, init_prod_r=4, init_prod_bit0=-1, init_prod_group=b, implied_zeros=0)
    assert np.array_equal(amp0, amp) and norm0 == norm and np.array_equal(counts0, counts)


@pytest.mark.parametrize("W,r,b", [(14, 6, 4), (16, 6, 3), (14, 4, 4)])
def test_fewer_tiles_than_a_group(W, r, b):
    """2^14 / 64 / 256 = 1 tile, 2^16 / 64 / 256 = 4, 2^14 / 16 / 256 = 4: B falls back to what the tile index has"""
    zero = [W - 1]
    _check(_ops(W, zero, _random_factors(W, zero, 12, seed=W + r), seed=r), W=W, init_prod_r=r, init_prod_bit0=-1,
           init_prod_group=b)


@pytest.mark.parametrize("grid", [1, 3, 5])
@pytest.mark.parametrize("b", [1, 2, -1])
def test_grid_not_a_divisor(b, grid):
    zero = [15]
    _check(_ops(16, zero, _random_factors(16, zero, 12, seed=grid), seed=grid), init_prod_r=4, init_prod_bit0=-1,
           init_prod_grid=grid, init_prod_group=b)


@pytest.mark.parametrize("devices", [1, 2, 4])
@pytest.mark.parametrize("bit0", [0, -1])
def test_virtual_shards(devices, bit0):
    zero = [15]
    _check(_ops(16, zero, _random_factors(16, zero, 14, seed=devices), seed=devices), devices=devices,
           init_prod_bit0=bit0)
