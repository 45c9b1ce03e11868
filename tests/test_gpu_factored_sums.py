"""The factored tile sums (option sums_factored: k_prod_sums over the 2^|D| tiles the inner factors tell apart, then
k_tile_sums_expand).  As tests/test_gpu_tile_sums.py does, every case runs one program, reads Engine.tile_sums() and then
the amplitudes, and holds every tile's sum to math.fsum of |amp|^2 over the tile's addresses within
_tile_sum_model.bound, (9 nfac + 2^R + 32) 2^-53 -- the factored order keeps that bound: _factored_sum_model derives
it and tests/test_factored_sum_model.py holds the numpy restatement to it on these programs.  Zero tiles are exactly
0.0, the engine's total is the norm, one init_prod launch with 0 bytes is booked, and Engine.tile_sums_info() must
report the path, |D| and the factor split of the host model (_factored_sum_model.info).

The programs are _factored_sum_model.CASES; W = 16, R = 4, init_prod_bit0 = -1 has block bits 7..10 (16 tiles)."""
import math

import numpy as np
import pytest

import _factored_sum_model as fm
import _tile_sum_model as tm
from _sampler_reference import TOL_REL, check_inverse_cdf, sorted_uniforms, unshuffle
from test_gpu_generator import FACTOR_LISTS as LISTS_A
from test_gpu_generator_groups import FACTOR_LISTS as LISTS_B

pytestmark = pytest.mark.gpu


def _ops(c):
    from qcmrf_amd import ir
    mask = (1 << c["w"]) - 1
    for q in c["zero"]:
        mask &= ~(1 << q)
    tables = fm.tables_for(c["factors"], c["seed"], c["overrides"])
    return [ir.op_init(mask)] + [ir.op_diag(qs, t) for qs, t in zip(c["factors"], tables)]


def _check(c, devices=1, defer=1, factored=1, **opts):
    """one run: (tile sums per shard, amplitudes)"""
    from qcmrf_amd import _lib, program
    rec, data = program.encode(_ops(c))
    w = c["w"]
    eng = _lib.Engine(w, devices=(0,) * devices)
    try:
        for k, v in dict(opts, init_prod_r=c["r"], init_prod_bit0=c["bit0"], defer_state=defer, sums_factored=factored).items():
            eng.set_option(k, v)
        eng.reset_stats()
        eng.exec(rec, data)
        sums = [eng.tile_sums(s) for s in range(devices)]
        infos = [eng.tile_sums_info(s) for s in range(devices)]
        norm = eng.norm()
        info = eng.state_info()
        kinds = eng.stats()["kinds"]
        amp = eng.amplitudes()
    finally:
        eng.close()
    assert info["deferred"] == bool(defer) and info["realize_calls"] == 0, info
    assert set(kinds) == {"init_prod"} and kinds["init_prod"]["launches"] == devices, kinds
    assert (kinds["init_prod"]["bytes"] == 0.0) == bool(defer), kinds
    L = w - (devices.bit_length() - 1)
    regs, _, block = tm.geometry(L, c["r"], c["bit0"])
    local = [[q for q in qs if q < L] for qs in c["factors"]]
    want_info = fm.info(L, c["r"], c["bit0"], c["zero"], [qs for qs in local if qs], factored)
    rel = tm.bound(len(c["factors"]), len(regs))
    total = 0.0
    for s in range(devices):
        assert infos[s] == want_info, (s, infos[s], want_info)
        want = tm.exact_tile_sums(amp[s << L:(s + 1) << L], block)
        got = sums[s]
        assert got.shape == want.shape
        err = np.abs(got - want)
        worst = float((err / np.where(want > 0, want, 1.0)).max())
        print("shard %d: %d tiles, %s, worst relative error %.3g of bound %.3g" % (s, got.size, infos[s], worst, rel))
        assert (err <= rel * want).all(), (s, worst, rel)
        assert (got[want == 0.0] == 0.0).all()
        total += tm.engine_total(got)
    assert total == norm, (total, norm)
    return sums, amp


def _same(a, b):
    assert len(a) == len(b) and all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("name", sorted(fm.CASES))
def test_every_program(name):
    """factored against the exact sums; the amplitudes are the same bits with sums_factored 1 and 0"""
    c = fm.CASES[name]
    opts = dict(pass_max_ops=512) if len(c["factors"]) > 56 else {}
    s1, a1 = _check(c, factored=1, **opts)
    s0, a0 = _check(c, factored=0, **opts)
    assert a1.tobytes() == a0.tobytes()
    if name == "d4_no_uniform":
        _same(s1, s0)                                  # D is every tile bit and nothing is tile-uniform: today's launch


@pytest.mark.parametrize("name,factored", [("d0", True), ("d1", True), ("d2", False)])
def test_auto_takes_it_from_three_removed_bits(name, factored):
    c = fm.CASES[name]
    assert fm.info(16, 4, -1, c["zero"], c["factors"], -1)["factored"] == factored
    _same(_check(c, factored=-1)[0], _check(c, factored=int(factored))[0])


@pytest.mark.parametrize("b", [0, 1, 2, 3, 4, -1])
@pytest.mark.parametrize("name", ["d0", "d2", "d3"])
def test_group_bits(name, b):
    """requests for more group bits than |D| has included"""
    _check(fm.CASES[name], init_prod_group=b)


@pytest.mark.parametrize("name", sorted(k for k in fm.CASES if k.startswith("zero_")))
def test_implied_zeros_do_not_matter(name):
    c = fm.CASES[name]
    _same(_check(c, implied_zeros=1)[0], _check(c, implied_zeros=0)[0])


def test_exact_zero_tiles():
    sums, _ = _check(fm.CASES["zero_uniform_entry"])
    assert (sums[0][[t for t in range(16) if t & 2]] == 0.0).all() and (sums[0] > 0).sum() == 8
    sums, _ = _check(fm.CASES["zero_inner_entry"])
    assert (sums[0] > 0).all()


def _mixed(free10):
    """the multi and mixed lists of the generator tests with tile-uniform factors added.  As they stand their inner
    factors touch every block bit (|D| = 4: the unfactored launch runs, and the info says so); free10 moves the one use
    of qubit 10 to qubit 9, so that D = {7, 8, 9} and the register-sum form of k_prod_sums (REGSUM) runs factored."""
    fl = LISTS_B["group_and_register"] + [[8]] + LISTS_A["multi_register"] + [[7, 10]]
    if free10:
        assert [8, 10, 12, 13] in fl
        fl = [[8, 9, 12, 13] if qs == [8, 10, 12, 13] else qs for qs in fl] + [[10]]
    return fm.case(factors=fl, seed=16)


@pytest.mark.parametrize("b", [4, -1])
@pytest.mark.parametrize("free10", [False, True])
def test_multi_and_mixed_lists(free10, b):
    c = _mixed(free10)
    assert fm.info(16, 4, -1, c["zero"], c["factors"], 1)["factored"] == free10
    _check(c, init_prod_group=b)


@pytest.mark.parametrize("name,b", [("d2", 2), ("d3", -1), ("w20", -1)])
def test_grid_does_not_matter(name, b):
    c = fm.CASES[name]
    s, _ = _check(c, init_prod_group=b)
    for grid in (1, 3):
        _same(s, _check(c, init_prod_group=b, init_prod_grid=grid)[0])


@pytest.mark.parametrize("devices", [2, 4])
def test_virtual_shards(devices):
    zero = [13]                                        # a register bit of every shard size here
    fl = fm.random_factors(14, zero + [8], 12, seed=devices) + [[8], [8]]  # local qubits only; 8 is a block bit of both sizes
    c = fm.case(w=16, r=4, bit0=-1, zero=zero, factors=fl, seed=devices)
    assert fm.info(16 - devices // 2, 4, -1, zero, fl, 1)["factored"]
    _check(c, devices=devices)


@pytest.mark.parametrize("name", ["d1", "d3", "w18"])
def test_deferred_or_written_the_same_sums(name):
    c = fm.CASES[name]
    _same(_check(c, defer=1)[0], _check(c, defer=0)[0])


@pytest.mark.parametrize("name", ["d2", "zero_uniform_entry", "mixed"])
def test_sampling_from_these_sums(name):
    """3000 shots from the factored and from the unfactored sums, each held to the order-free inverse-CDF contract over
    the read-back |amp|^2.  The sums differ by ulps, so the words are compared and the outcome printed, not asserted."""
    from qcmrf_amd import _lib, program
    c = _mixed(True) if name == "mixed" else fm.CASES[name]
    rec, data = program.encode(_ops(c))
    shots, seed = 3000, 11
    words = []
    for factored in (1, 0):
        eng = _lib.Engine(16)
        try:
            for k, v in dict(init_prod_r=4, init_prod_bit0=-1, defer_state=1, sums_factored=factored).items():
                eng.set_option(k, v)
            eng.exec(rec, data)
            assert eng.tile_sums_info()["factored"] == bool(factored)
            total = eng.norm()
            x = unshuffle(seed, shots, eng.sample(shots, seed))
            assert eng.state_info()["deferred"]
            p = np.abs(eng.amplitudes()) ** 2
            assert abs(total - math.fsum(p.tolist())) <= TOL_REL * total
            assert check_inverse_cdf(p, sorted_uniforms(seed, shots, total), x, TOL_REL * total, total) == [], (name, factored)
            words.append(x)
        finally:
            eng.close()
    print("%s: %d of %d words differ between sums_factored 1 and 0" % (name, int((words[0] != words[1]).sum()), shots))


def test_info_needs_the_generator_sums():
    from qcmrf_amd import _lib
    eng = _lib.Engine(14)
    try:
        eng.init_uniform((1 << 14) - 1)
        with pytest.raises(ValueError):
            eng.tile_sums_info()
    finally:
        eng.close()
