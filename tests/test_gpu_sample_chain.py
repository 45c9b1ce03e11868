"""Option sample_chain: qsv_sample with the super-sum walk on the device (k_walk_super, k_walk_shots) and, on a deferred
shard, every shot located inside the generator (form QSV_GEN_LOCATE of k_init_prod), against sample_chain = 0 -- the host
walk, the listed tiles stored and read back by k_locate_tile.  One engine, one seed, the option alone changes: the 64-bit
words must be equal one by one.  The arithmetic of the walk is pinned on the host by tests/test_sample_chain_model.py.

Programs: an init and diagonal factors only (the generator is the only pass), from tests/_deferred_cases.py and
tests/_factored_sum_model.py, at 14-18 qubits with defer_state = 1, and twice at 29 / 30 qubits, where the shard is
allocated and never written."""
import numpy as np
import pytest

import _deferred_cases as dc
import _factored_sum_model as fm

pytestmark = pytest.mark.gpu

SEED = 23
PERM16 = [5, 0, 15, 9, 3, 12, 7, 1, 14, 2, 11, 8, 4, 13, 6, 10]
HOLES = [9, -1, 3, 15, -1, -1, 0, 12, 7]


def _fm_ops(c):
    from qcmrf_amd import ir
    mask = (1 << c["w"]) - 1
    for q in c["zero"]:
        mask &= ~(1 << q)
    tables = fm.tables_for(c["factors"], c["seed"], c["overrides"])
    return [ir.op_init(mask)] + [ir.op_diag(qs, t) for qs, t in zip(c["factors"], tables)]


def _engine(ops, w, devices=1, defer=1, **opts):
    from qcmrf_amd import _lib, program
    rec, data = program.encode(ops)
    eng = _lib.Engine(w, devices=(0,) * devices)
    for k, v in dict(opts, defer_state=defer).items():
        eng.set_option(k, v)
    eng.exec(rec, data)
    return eng, (rec, data)


def _pair(eng, runs, deferred=True, chain_taken=True):
    """every (shots, meas_qubits) of ``runs`` with sample_chain 0, then 1: equal words; the state stays as it was"""
    out = []
    for shots, meas in runs:
        eng.set_option("sample_chain", 0)
        w0 = eng.sample(shots, SEED, meas)
        eng.sample(shots, SEED + 1, meas)               # other words in the result buffer: a kernel that wrote nothing would show
        before = eng.state_info()
        eng.set_option("sample_chain", 1)
        w1 = eng.sample(shots, SEED, meas)
        after = eng.state_info()
        diff = int((w0 != w1).sum())
        print("%d shots, meas %s: %d words differ" % (shots, "all" if meas is None else len(meas), diff))
        assert w0.dtype == np.uint64 and w0.shape == w1.shape == (shots,)
        assert diff == 0
        assert after["deferred"] == deferred and after["realize_calls"] == before["realize_calls"], (before, after)
        if deferred and chain_taken:
            assert after["listed_launches"] == before["listed_launches"] + 1, (before, after)
        out.append(w0)
    return out


def _check(ops, w, runs, devices=1, defer=1, **opts):
    eng, prog = _engine(ops, w, devices, defer, **opts)
    try:
        assert eng.state_info()["deferred"] == bool(defer)
        words = _pair(eng, runs, deferred=bool(defer), chain_taken=devices == 1)
        # ... and on a fresh state, where the chain forms the super sums itself (above, sample_chain = 0 left them behind)
        shots, meas = runs[-1]
        eng.set_option("sample_chain", 0)
        eng.sample(shots, SEED + 1, meas)
        eng.exec(*prog)
        eng.set_option("sample_chain", 1)
        assert np.array_equal(eng.sample(shots, SEED, meas), words[-1])
        return words
    finally:
        eng.close()


RUNS = [(1, None), (2, PERM16), (4096, None), (4096, PERM16), (4096, HOLES)]


@pytest.mark.parametrize("r", [3, 4, 5, 6])
def test_every_tile_width_and_group(r):
    """R = 3..6 with 0..4 group bits on the top bits, and the other two register placements with the automatic group"""
    c = fm.CASES["r%d_bit-1" % r]
    for group in (0, 1, 2, 3, 4):
        _check(_fm_ops(c), c["w"], RUNS if group == 3 else RUNS[2:3] + RUNS[:1], init_prod_r=r, init_prod_bit0=-1,
               init_prod_group=group)
    for bit0 in (0, 8):
        c = fm.CASES["r%d_bit%d" % (r, bit0)]
        _check(_fm_ops(c), c["w"], RUNS[3:], init_prod_r=r, init_prod_bit0=bit0)


@pytest.mark.parametrize("group", [0, 2])
def test_peaked_on_one_tile(group):
    """nearly all the mass in tile 5 of 16: hundreds of shots share a tile, entry after entry of the list is equal"""
    peak = np.full(16, 0.01, dtype=np.complex128)
    peak[5] = 1.0
    factors = [dc.BLOCK] + dc.random_factors(dc.W, [dc.REG_BIT], 10, seed=3)
    ops = dc.program_ops(dc.W, [dc.REG_BIT], factors, seed=4, tables={0: peak})
    words = _check(ops, dc.W, RUNS[2:], init_prod_r=4, init_prod_bit0=-1, init_prod_group=group)
    tile = sum(((words[0] >> np.uint64(q)) & np.uint64(1)) << np.uint64(i) for i, q in enumerate(dc.BLOCK))
    assert (tile == 5).sum() > 3500


@pytest.mark.parametrize("name", ["zero_uniform_entry", "zero_inner_entry", "zero_15", "zero_3", "zero_5", "zero_9", "zero_8",
                                  "zero_None", "d3", "hundred", "w18"])
def test_zeros_and_factor_classes(name):
    """tiles whose sum is exactly 0 (a zero table entry on a block bit), a provably-zero qubit on a register, lane, wave
    and block bit, mixed and multi-register factors, two descriptors per lane, 18 qubits"""
    c = fm.CASES[name]
    opts = dict(pass_max_ops=512) if len(c["factors"]) > 56 else {}
    meas = list(range(c["w"]))[::-1]
    for group in (-1, 4):
        _check(_fm_ops(c), c["w"], [(4096, None), (4096, meas), (2, HOLES)], init_prod_r=c["r"], init_prod_bit0=c["bit0"],
               init_prod_group=group, **opts)


@pytest.mark.parametrize("w", [14, 15, 17])
def test_other_sizes(w):
    _check(dc.default_ops(seed=w, zero=(w - 1,), w=w), w, [(4096, None), (1, None)], init_prod_r=4, init_prod_bit0=-1)


def test_more_shots_than_a_grid_holds():
    """70 000 shots at 14 qubits: past the 65 535 workgroups of the one-workgroup-per-shot launches"""
    _check(dc.default_ops(seed=2, zero=(13,), w=14), 14, [(70000, None)], init_prod_r=4, init_prod_bit0=-1)


@pytest.mark.parametrize("w", [29, 30])
def test_large_shard_never_written(w):
    """2^17 / 2^18 tile sums, 128 / 256 super sums: past the 64-entry leaf of the total's pairwise association"""
    _check(dc.default_ops(seed=w, zero=(w - 1,), n=14, w=w), w, [(4096, None)], init_prod_r=4)


def test_zero_norm_is_the_same_error():
    factors = dc.random_factors(dc.W, [dc.REG_BIT], 6, seed=5)
    ops = dc.program_ops(dc.W, [dc.REG_BIT], factors, seed=6, tables={2: np.zeros(2 ** len(factors[2]))})
    eng, _ = _engine(ops, dc.W, init_prod_r=4, init_prod_bit0=-1)
    try:
        msgs = []
        for chain in (0, 1):
            eng.set_option("sample_chain", chain)
            with pytest.raises(Exception) as e:
                eng.sample(100, SEED)
            msgs.append((type(e.value), str(e.value)))
        assert msgs[0] == msgs[1] and "zero norm" in msgs[0][1], msgs
    finally:
        eng.close()


def test_stored_state_keeps_k_locate_tile():
    """defer_state = 0: the walk on the device, the shots located in the stored amplitudes"""
    c = fm.CASES["zero_3"]
    _check(_fm_ops(c), c["w"], RUNS[2:], defer=0, init_prod_r=4, init_prod_bit0=-1)
    _check(dc.default_ops(), dc.W, RUNS[2:4], defer=0)


def test_two_shards_take_the_host_walk():
    """a handle with two shards is outside the chain: the option changes nothing"""
    eng, _ = _engine(dc.default_ops(seed=3, zero=()), dc.W, devices=2, init_prod_r=4, init_prod_bit0=-1)
    try:
        listed = []
        words = []
        for chain in (0, 1):
            eng.set_option("sample_chain", chain)
            n0 = eng.state_info()["listed_launches"]
            words.append(eng.sample(4096, SEED))
            listed.append(eng.state_info()["listed_launches"] - n0)
        assert np.array_equal(words[0], words[1])
        assert listed[0] == listed[1] >= 1, listed
    finally:
        eng.close()
