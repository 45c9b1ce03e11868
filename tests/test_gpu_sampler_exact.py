"""qsv_sample shot by shot against the exact inverse-CDF reference (_sampler_reference.py).

The uniforms of a call are rebuilt from the seed and the engine's own total, the final shuffle is undone, and every
word is held against the uniform that drew it:

  index-order path (k_locate over block sums, states loaded with set_amplitudes): every word equals the reference's
    first index whose prefix sum exceeds the uniform -- test_sampler_reference.py has shown that none of these
    uniforms lies within the tolerance of a prefix boundary, and this file asserts it again for the engine's total;
  tile-order path (k_locate_super + k_locate_tile over the tile sums of the program's last pass): the walk order
    belongs to the pass, so the words are held to the order-free contract (check_inverse_cdf) over |amplitudes|^2 read
    back after the run -- which first has to match the numpy engine within the suite's 1e-12 -- and, with
    fused_sums = 0, again to word equality.

Which path ran is read from the engine's statistics: a QSV_K_PROB launch (the block-sum read pass) happens on the
index-order path only."""
import math

import numpy as np
import pytest

import _sampler_cases as sc
from _sampler_reference import TOL_REL, check_inverse_cdf, exact_index_order, sorted_uniforms, unshuffle

pytestmark = pytest.mark.gpu

SUM_SLACK = 2.5e-13        # the engine's total against fsum(p): the bound on its summation chains (reference docstring)


@pytest.fixture(scope="module")
def lib():
    from qcmrf_amd import _lib
    _lib.load()
    assert _lib.device_count() >= 1
    return _lib


def _draw(eng, shots, seed):
    """one call: (total, r, x, QSV_K_PROB launches of norm + sample) with x[s] the word drawn for r[s]"""
    eng.reset_stats()
    total = eng.norm()
    words = eng.sample(shots, seed)
    assert words.dtype == np.uint64 and len(words) == shots
    prob = eng.stats()["kinds"].get("prob", {}).get("launches", 0)
    return total, sorted_uniforms(seed, shots, total), unshuffle(seed, shots, words), prob


def _assert_exact(p, total, r, x, what):
    """every word equals the index-order reference; nothing near a boundary, nothing skipped"""
    tol = TOL_REL * total
    assert abs(total - math.fsum(p.tolist())) <= SUM_SLACK * total, what
    want, dist = exact_index_order(p, r)
    assert int((dist <= tol).sum()) == 0, (what, float(dist.min()))
    bad = np.flatnonzero(x != want)
    assert bad.size == 0, (what, bad.size, bad[:5].tolist(), x[bad[:5]].tolist(), want[bad[:5]].tolist())
    assert check_inverse_cdf(p, r, x, tol, total) == [], what


# ---------------------------------------------------------------------------------------------------------------------
# index-order path
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in sorted(sc.INDEX_CASES) if n != "invalidation"])
def test_index_order_words(lib, name):
    """sub-block shard, empty first / last block (the host's last_nz clamp), empty rows, empty shards among four
    (last_shard, shard bits in the words), 100 then 70 000 shots on one engine (buffer growth past 8192, more than
    65 535 shots in one shard: the grid-stride loop of k_locate), one populated index, 2^-40 of the mass in block 0 and
    the rest on the last amplitude, 0 / 1 / 2 shots, an unnormalised state"""
    n, P, steps = sc.INDEX_CASES[name]
    with lib.Engine(n, devices=(0,) * P) as eng:
        for state, calls in steps():
            eng.set_amplitudes(0, state)
            p = sc.probs(state)
            first = True
            for shots, seed in calls:
                total, r, x, prob = _draw(eng, shots, seed)
                assert (prob > 0) == first, (name, shots, prob)      # one read pass per state: the block sums are cached
                first = False
                if shots:
                    _assert_exact(p, total, r, x, (name, shots, seed))
    if name == "heavy_shard_buffer_growth":
        assert int((x < (1 << (n - 1))).sum()) > 65535               # the case is what it claims to be
    if name == "shards_1_3_empty":
        assert set((x >> np.uint64(12)).tolist()) == {0, 2}
    if name == "last_amp_plus_tiny":
        assert (x == (1 << n) - 1).all()


def test_index_order_follows_the_resident_state(lib):
    """sample, load another state, sample, apply a gate, sample: each call draws from the state then resident (cached
    block sums dropped by set_amplitudes and by the gate)"""
    n, P, steps = sc.INDEX_CASES["invalidation"]
    (a, ca), (b, cb), (c, cc) = steps()
    with lib.Engine(n) as eng:
        for state, calls, gate in ((a, ca, False), (b, cb, False), (c, cc, True)):
            if gate:
                eng.apply_1q(sc.INVALIDATION_T, sc.INVALIDATION_U)
                assert np.abs(eng.amplitudes() - state).max() < 1e-13
            else:
                eng.set_amplitudes(0, state)
            (shots, seed), = calls
            total, r, x, prob = _draw(eng, shots, seed)
            assert prob > 0
            _assert_exact(sc.probs(state), total, r, x, ("invalidation", seed))
        assert int((x & np.uint64(1 << sc.INVALIDATION_T) != 0).sum()) > 0      # the gate populated qubit 5


def _remap(raw, meas):
    out = np.zeros(len(raw), dtype=np.uint64)
    for j, q in enumerate(meas):
        if q >= 0:
            out |= ((raw >> np.uint64(q)) & np.uint64(1)) << np.uint64(j)
    return out


def test_remap_bits(lib):
    """k_remap_bits: sample(shots, seed, meas) is the bit remap of sample(shots, seed) -- unwritten (-1) entries, shard
    bits (12, 13 of 4 shards), a qubit read into several classical bits, all 64 entries in use"""
    n, P = 14, 4
    state = sc.rand_state(n, 91)
    lists = {
        "plain": [7, 1, 3],
        "unwritten": [3, -1, 0, -1, -1, 9],
        "shard_bits": [13, 12, 0, 11],
        "shard_bits_unwritten_first": [-1, 13, -1, 12],
        "all_64": [(5 * j) % n if j % 3 != 2 else -1 for j in range(64)],
        "bit_63_only": [-1] * 63 + [13],
    }
    shots, seed = 3000, 92
    with lib.Engine(n, devices=(0,) * P) as eng:
        eng.set_amplitudes(0, state)
        raw = eng.sample(shots, seed)
        assert len(set((raw >> np.uint64(12)).tolist())) == 4
        for name, meas in lists.items():
            assert np.array_equal(eng.sample(shots, seed, meas), _remap(raw, meas)), name
        assert np.array_equal(eng.sample(shots, seed), raw)


# ---------------------------------------------------------------------------------------------------------------------
# tile-order path
# ---------------------------------------------------------------------------------------------------------------------
def _run_program(lib, name, opts, expect_tile=True, expect_kind=None):
    """the program under ``opts`` with fused_sums 1 (contract; the tile path must have run if ``expect_tile``) and 0
    (word equality).  Returns the amplitudes read back in the fused run."""
    W, P, _, shots, seed = sc.TILE_PROGRAMS[name]
    rec, data, want = sc.tile_reference(name)
    out = None
    for fused in (1, 0):
        with lib.Engine(W, devices=(0,) * P) as eng:
            for k, v in dict(opts, fused_sums=fused).items():
                eng.set_option(k, v)
            eng.set_amplitudes(0, np.full(1 << W, 1.0 + 1.0j))     # whatever the program does not write is not zero
            eng.reset_stats()
            eng.exec(rec, data)
            if expect_kind:
                assert eng.stats()["kinds"].get(expect_kind, {}).get("launches", 0) >= 1, (name, opts)
            got = eng.amplitudes()
            assert np.abs(got - want).max() < 1e-12, (name, opts, fused)      # the gates are not what is under test
            p = sc.probs(got)
            total, r, x, prob = _draw(eng, shots, seed)
            tol = TOL_REL * total
            assert abs(total - math.fsum(p.tolist())) <= SUM_SLACK * total, (name, opts, fused)
            assert check_inverse_cdf(p, r, x, tol, total) == [], (name, opts, fused)
            if fused:
                assert (prob == 0) == expect_tile, (name, opts, prob)
                if expect_tile:        # a tile holds register bits above the lane bits: its walk is not the index walk,
                    assert (x != exact_index_order(p, r)[0]).any(), (name, opts)      # so the contract is what holds here
                out = got
            else:
                assert prob > 0, (name, opts)
                _assert_exact(p, total, r, x, (name, opts))
    return out


@pytest.mark.parametrize("zero_tracking", [0, 1])
@pytest.mark.parametrize("dyn_lanes", [0, 3])
@pytest.mark.parametrize("lane_map", [0, 1])
@pytest.mark.parametrize("multi_r", [1, 2, 3, 4, 5, 6])
def test_tile_order_every_tile_width(lib, multi_r, lane_map, dyn_lanes, zero_tracking):
    """k_locate_tile<R> for every R a last pass can have, with and without the lane map, borrowed lanes and zero
    tracking (qubit 15 stays |0>: under zero tracking the last pass enumerates half the tiles and zmask != 0)"""
    _run_program(lib, "general_and_table", {"multi_r": multi_r, "lane_map": lane_map, "lane_map_min_l": 14,
                                            "dyn_lanes": dyn_lanes, "zero_tracking": zero_tracking})


def test_tile_order_more_shots_than_workgroups(lib):
    """70 000 shots on the tile path: the staging buffers grow past 8192 and the grid of k_locate_super and
    k_locate_tile (65 535 workgroups at most) walks more than one shot per workgroup"""
    _run_program(lib, "general_and_table_70000_shots", {})


@pytest.mark.parametrize("xframe", [1, 0])
@pytest.mark.parametrize("name,tile", [("trailing_x_register_bit", True), ("trailing_x_lane_bit", True),
                                       ("trailing_x_block_bit", False), ("init_pass_with_x", True)])
def test_tile_order_through_the_x_frame(lib, name, tile, xframe):
    """an uncontrolled X at the end of the program rides in the last pass's store addresses (tile_xor != 0) on a
    register or lane bit.  On a block bit of a pass that reads, it cannot: it runs as a swap after the pass, which drops
    the tile sums (index-order path); a write-only pass takes it on any bit (init_pass_with_x).  xframe 0: the X is an
    op of the pass like any other."""
    _run_program(lib, name, {"xframe": xframe}, expect_tile=tile or not xframe)


@pytest.mark.parametrize("group", [-1, 0])
@pytest.mark.parametrize("implied_zeros", [1, 0])
@pytest.mark.parametrize("P", [1, 2])
def test_tile_order_after_the_generator(lib, P, implied_zeros, group):
    """k_init_prod as the last pass, the top local qubit left |0>: with implied zeros that half of every shard is never
    written and k_locate_tile must not load it (zmask != 0): _run_program fills the state with 1 + i first, so a
    load would show"""
    name = "generator_P%d" % P
    got = _run_program(lib, name, {"implied_zeros": implied_zeros, "init_prod_group": group}, expect_kind="init_prod")
    top = 16 - (P.bit_length() - 1) - 1
    assert not got[(np.arange(got.size) >> top) & 1 == 1].any()


@pytest.mark.parametrize("name", ["four_super_blocks_upper_empty", "four_super_blocks_lower_empty"])
def test_tile_order_four_super_blocks(lib, name):
    """2^22 amplitudes at R = 2: 4096 tiles, so the host walks four super sums and k_locate_super the tiles of one.
    Upper half empty: the last two super blocks carry nothing (the host's clamp to the last populated one and the
    kernel's to the last populated tile); lower half empty: the first two."""
    got = _run_program(lib, name, {"multi_r": 2})
    half = got.size // 2
    empty = got[half:] if name.endswith("upper_empty") else got[:half]
    assert not empty.any()


@pytest.mark.parametrize("seed", [11, 12])
def test_random_programs_sampled(seed):
    """scripts/stress_random_programs.py with sample_shots: every random tile layout (tile width, borrowed lanes, lane
    map, X frame, generator on / off, 1 / 2 / 4 shards) also draws 4096 shots that must satisfy the contract, and equal
    the index-order reference where fused_sums is 0"""
    import importlib.util
    import os
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("stress_random_programs", os.path.join(ROOT, "scripts", "stress_random_programs.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.run(60, seed, verbose=False, sample_shots=4096) == 0
