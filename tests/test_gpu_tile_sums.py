"""k_prod_sums: the generator's tile sums formed from the factors' |.|^2, without an amplitude.  Every case runs the
program deferred, reads Engine.tile_sums() while the state is still deferred (the accessor realises nothing), then
reads the amplitudes and holds every tile's sum to math.fsum of |amp|^2 over the tile's addresses.

Tile index = the block bits of the shard's address compacted in ascending order (_tile_sum_model.geometry restates
flush_init_product_r's choice of register, thread and block bits; at W = 16, R = 4, init_prod_bit0 = -1 the block
bits are 7..10).

Bound, relative to the tile's exact sum: (9 nfac + 2^R + 32) 2^-53 (_tile_sum_model.bound).  |stored amplitude|^2
carries 3 ulp per complex multiply twice (6 nfac); the kernel's term is a product of nfac weights fma(re, re, im im),
2 ulp each plus 1 per multiply (3 nfac); then one ulp per addition of non-negative terms along the longest chain:
the register sum -- R two-term sums multiplied together when only single-register factors touch the register bits,
else a pairwise tree of R levels over 2^R terms -- then 6 levels within the wave (l ^ 32, l ^ 16, l ^ 1, l ^ 2, half
row, row) and 2 for the four waves: fewer than 2^R + 32.  Derived, not fitted to a run."""
import math

import numpy as np
import pytest

import _tile_sum_model as tm
from _deferred_cases import program_ops, random_factors
from _sampler_reference import TOL_REL, check_inverse_cdf, sorted_uniforms, unshuffle
from test_gpu_generator import FACTOR_LISTS as LISTS_A, MAXLIST
from test_gpu_generator_groups import FACTOR_LISTS as LISTS_B

pytestmark = pytest.mark.gpu

TOP = dict(init_prod_r=4, init_prod_bit0=-1)


def _run(ops, w=16, devices=1, defer=1, **opts):
    """(tile sums per shard read while deferred, norm, amplitudes, info before the amplitudes were read, kinds)"""
    from qcmrf_amd import _lib, program
    rec, data = program.encode(ops)
    eng = _lib.Engine(w, devices=(0,) * devices)
    try:
        for k, v in opts.items():
            eng.set_option(k, v)
        eng.set_option("defer_state", defer)
        eng.reset_stats()
        eng.exec(rec, data)
        sums = [eng.tile_sums(s) for s in range(devices)]
        norm = eng.norm()
        info = eng.state_info()
        kinds = eng.stats()["kinds"]
        amp = eng.amplitudes()
        return sums, norm, amp, info, kinds
    finally:
        eng.close()


def _check(ops, w=16, devices=1, **opts):
    nfac = len(ops) - 1
    sums, norm, amp, info, kinds = _run(ops, w, devices, **opts)
    assert info["deferred"] and info["realize_calls"] == 0, info
    assert set(kinds) == {"init_prod"} and kinds["init_prod"]["launches"] == 1 * devices and kinds["init_prod"]["bytes"] == 0.0, kinds
    L = w - (devices.bit_length() - 1)
    regs, _, block = tm.geometry(L, opts.get("init_prod_r", 0), opts.get("init_prod_bit0", 0))
    rel = tm.bound(nfac, len(regs))
    total = 0.0
    for s in range(devices):
        want = tm.exact_tile_sums(amp[s << L:(s + 1) << L], block)
        got = sums[s]
        assert got.shape == want.shape
        err = np.abs(got - want)
        worst = float((err / np.where(want > 0, want, 1.0)).max())
        print("shard %d: %d tiles, worst relative error %.3g of bound %.3g" % (s, got.size, worst, rel))
        assert (err <= rel * want).all(), (s, worst, rel)
        assert (got[want == 0.0] == 0.0).all()
        total += tm.engine_total(got)
    assert total == norm, (total, norm)
    return sums


def _same(a, b):
    assert len(a) == len(b) and all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("bit0", [0, -1, 8])
@pytest.mark.parametrize("r", [3, 4, 5, 6])
def test_every_tile_width_and_placement(r, bit0):
    zero = [15]
    _check(program_ops(16, zero, random_factors(16, zero, 14, seed=r), seed=r + 50), init_prod_r=r, init_prod_bit0=bit0)


@pytest.mark.parametrize("b", [0, 1, 2, 3, 4, -1])
def test_group_bits(b):
    zero = [15]
    _check(program_ops(16, zero, random_factors(16, zero, 14, seed=20 + b), seed=b + 60), init_prod_group=b, **TOP)


@pytest.mark.parametrize("zq", [15, 3, 5, 9, None])
def test_zero_qubit_placement(zq):
    """the zero qubit on a register, lane, wave and block bit, and none; implied zeros on and off: the same sums"""
    zero = [] if zq is None else [zq]
    ops = program_ops(16, zero, random_factors(16, zero, 16, seed=zq or 0), seed=3)
    s1 = _check(ops, implied_zeros=1, **TOP)
    s0 = _check(ops, implied_zeros=0, **TOP)
    _same(s0, s1)


def _lists():
    out = {}
    for k, v in LISTS_A.items():
        if v is None:
            rs = np.random.RandomState(1)
            v = [[int(q) for q in rs.choice(range(15), size=n, replace=False)] for n in range(1, MAXLIST + 1)]
        out["a_" + k] = v
    out.update({"b_" + k: v for k, v in LISTS_B.items()})
    return out


@pytest.mark.parametrize("b", [4, -1])
@pytest.mark.parametrize("name", sorted(_lists()))
def test_factor_lists(name, b):
    """the shapes of both generator test files: multi_register and group_and_register are the multi and mixed paths"""
    _check(program_ops(16, [15], _lists()[name], seed=7), init_prod_group=b, **TOP)


def test_100_factors():
    """factors 64.. sit on the second descriptor lane"""
    zero = [15]
    _check(program_ops(16, zero, random_factors(16, zero, 100, seed=2, kmax=3), seed=4), pass_max_ops=512, **TOP)


def test_tables_at_lds_limit():
    rs = np.random.RandomState(9)
    fl = [[int(q) for q in rs.choice(range(15), size=k, replace=False)] for k in (10, 10, 8, 7, 6, 5, 4, 3, 2)]
    assert sum(2 ** len(qs) for qs in fl) == 2556
    _check(program_ops(16, [15], fl, seed=8), **TOP)


@pytest.mark.parametrize("w,r,b", [(14, 6, 4), (14, 4, 4), (18, 4, -1), (18, 4, 4)])
def test_tile_counts(w, r, b):
    """one tile (fewer than a group), 4, and 64 tiles (two chunks of a 16-tile group)"""
    zero = [w - 1]
    _check(program_ops(w, zero, random_factors(w, zero, 12, seed=w + r), seed=r), w=w, init_prod_r=r, init_prod_bit0=-1,
           init_prod_group=b)


@pytest.mark.parametrize("b", [2, -1])
def test_grid_does_not_matter(b):
    zero = [15]
    ops = program_ops(16, zero, random_factors(16, zero, 12, seed=5), seed=5)
    s = _check(ops, init_prod_group=b, **TOP)
    for grid in (1, 3):
        _same(s, _check(ops, init_prod_group=b, init_prod_grid=grid, **TOP))


@pytest.mark.parametrize("devices", [2, 4])
def test_virtual_shards(devices):
    zero = [13]                                        # a register bit of every shard size here
    _check(program_ops(16, zero, random_factors(16, zero, 14, seed=devices), seed=devices), devices=devices,
           init_prod_bit0=-1)


def _skewed():
    """a 1 : 1e-3 weight on every block bit, other factors around them"""
    fl = [[7], [8], [9], [10]] + random_factors(16, [15], 8, seed=12)
    tabs = {i: np.array([1.0, 10.0 ** -1.5 * np.exp(0.3j * (i + 1))]) for i in range(4)}
    return program_ops(16, [15], fl, seed=13, tables=tabs)


def _zero_tiles():
    """an exact 0 in a table wherever block bit 8 is set: those tiles sum to exactly 0.0"""
    fl = [[8, 2], [10, 8], [0, 12]] + random_factors(16, [15], 6, seed=14)
    t0 = np.array([0.7, 0.0, 0.9j, 0.0])                # index bit 0 <-> qubit 8: zero where bit 8 is set
    return program_ops(16, [15], fl, seed=15, tables={0: t0})


def _mixed():
    return program_ops(16, [15], LISTS_B["group_and_register"] + LISTS_A["multi_register"], seed=16)


def test_skewed_block_bits():
    _check(_skewed(), **TOP)


def test_exact_zero_tiles():
    sums = _check(_zero_tiles(), **TOP)
    assert (sums[0][[t for t in range(16) if t & 2]] == 0.0).all() and (sums[0] > 0).sum() == 8


@pytest.mark.parametrize("case", ["skewed", "mixed", "zero_tiles"])
def test_sampling_from_these_sums(case):
    """3000 shots deferred and not deferred: the same words, held to the order-free inverse-CDF contract over the
    read-back |amp|^2"""
    from qcmrf_amd import _lib, program
    ops = {"skewed": _skewed, "mixed": _mixed, "zero_tiles": _zero_tiles}[case]()
    rec, data = program.encode(ops)
    shots, seed = 3000, 11
    words = []
    for defer in (1, 0):
        eng = _lib.Engine(16)
        try:
            for k, v in dict(TOP, init_prod_group=4 if case == "mixed" else -1, defer_state=defer).items():
                eng.set_option(k, v)
            eng.exec(rec, data)
            total = eng.norm()
            x = unshuffle(seed, shots, eng.sample(shots, seed))
            assert eng.state_info()["deferred"] == bool(defer)
            p = np.abs(eng.amplitudes()) ** 2
            assert abs(total - math.fsum(p.tolist())) <= TOL_REL * total
            assert check_inverse_cdf(p, sorted_uniforms(seed, shots, total), x, TOL_REL * total, total) == [], (case, defer)
            words.append(x)
        finally:
            eng.close()
    assert np.array_equal(words[0], words[1])


def test_accessor_needs_valid_sums():
    from qcmrf_amd import _lib
    eng = _lib.Engine(14)
    try:
        eng.init_uniform((1 << 14) - 1)
        with pytest.raises(ValueError):
            eng.tile_sums()
    finally:
        eng.close()
