"""The slot primitives of the level-wise trajectory walk on the MI355X (qsv_branch_mass, qsv_branch_split; qsv_branch.hip)
against the numpy reference of _branch_reference.py: the split bit for bit, the sums within the project's sampling
tolerance of a longdouble sum, and bit for bit among themselves wherever the slot's contents are the same."""
import numpy as np
import pytest

import _branch_reference as br

pytestmark = pytest.mark.gpu

WIDTHS = [1, 3, 5, 6, 7, 8, 11, 12, 13, 14]
MASS_RTOL = 1e-12                 # sums of at most 2^W non-negative doubles


@pytest.fixture(scope="module")
def lib():
    from qcmrf_amd import _lib
    _lib.load()
    assert _lib.device_count() >= 1
    return _lib


def rand_slots(w, n_slots, seed, zero=()):
    """seeded complex-normal amplitudes, the slots of ``zero`` exactly zero"""
    rs = np.random.RandomState(seed)
    v = (rs.randn(n_slots << w) + 1j * rs.randn(n_slots << w)) / np.sqrt(2.0 * (n_slots << w))
    for b in zero:
        v[b << w: (b + 1) << w] = 0.0
    return v


def qubits_of(w):
    return sorted({q for q in (0, 3, 5, 6, w - 1) if 0 <= q < w})


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_mass(got, vec, w, n_slots, qubit):
    want = br.mass_array(vec, w, n_slots, qubit)
    assert got.shape == (n_slots, 2) and got.dtype == np.float64
    tot = (want[:, 0] + want[:, 1]).astype(np.float64)
    err = np.abs(got.astype(np.longdouble) - want).max(axis=1).astype(np.float64)
    assert (err <= MASS_RTOL * tot).all(), (w, qubit, float((err / np.maximum(tot, 1e-300)).max()))
    assert (got[tot == 0] == 0).all()


# children of the cases: (name, W_dst - w, parents, outcomes) on a source of 8 slots, slots 2 and 5 of it zero
def split_cases():
    return [("five of eight", 3, [7, 7, 3, 1, 0], [0, 1, 1, 0, 1]),          # a parent twice, parents absent, descending
            ("all eight", 3, [0, 1, 2, 3, 4, 5, 6, 7], [1, 0, 1, 1, 0, 0, 1, 0]),
            ("narrower", 1, [6, 2], [1, 0]),
            ("wider", 4, [4, 4, 5, 0, 3], [1, 0, 0, 1, 1]),
            ("one of many", 3, [5 + 1], [1]),
            ("extraction", 0, [3], [1])]


@pytest.mark.parametrize("w", WIDTHS)
def test_split_and_mass_against_numpy(lib, w):
    src_vec = rand_slots(w, 8, 1000 + w, zero=(2, 5))
    engines = {}
    with lib.Engine(w + 3) as src:
        src.set_amplitudes(0, src_vec)
        try:
            for d in (0, 1, 3, 4):
                engines[d] = lib.Engine(w + d)
                engines[d].set_amplitudes(0, rand_slots(w, 1 << d, 77 + d))      # a non-zero state before: stale slots must end zero
            for qubit in qubits_of(w):
                for n_slots in (1, 5, 8):
                    check_mass(src.branch_mass(w, n_slots, qubit), src_vec, w, n_slots, qubit)
                for release in (0, 1):
                    for name, d, parents, outcomes in split_cases():
                        dst = engines[d]
                        dst.branch_split(src, w, parents, outcomes, qubit, release)
                        want = br.split_array(src_vec, 1 << (w + d), w, parents, outcomes, qubit, release)
                        got = dst.amplitudes()
                        assert bits_equal(got, want), (name, w, qubit, release)
                        # the children's masses, on the destination: same shapes, the state written by the split
                        check_mass(dst.branch_mass(w, len(parents), qubit), want, w, len(parents), qubit)
            assert bits_equal(src.amplitudes(), src_vec)                          # the source intact afterwards
        finally:
            for e in engines.values():
                e.close()


def test_many_small_slots(lib):
    """1024 slots of w = 4: many workgroups, each of several slots (256 per workgroup of the split, 64 per wave of the sums)"""
    w, n = 4, 1024
    rs = np.random.RandomState(5)
    vec = rand_slots(w, n, 6, zero=(0, 17, 511, 1023))
    parents = rs.randint(0, n, size=n)
    parents[:4] = [1023, 1023, 0, 17]
    outcomes = rs.randint(0, 2, size=n)
    with lib.Engine(w + 10) as src, lib.Engine(w + 10) as dst, lib.Engine(w + 11) as big:
        src.set_amplitudes(0, vec)
        for qubit in (0, 3):
            check_mass(src.branch_mass(w, n, qubit), vec, w, n, qubit)
            check_mass(src.branch_mass(w, 1001, qubit), vec, w, 1001, qubit)
            for release in (0, 1):
                dst.branch_split(src, w, parents, outcomes, qubit, release)
                assert bits_equal(dst.amplitudes(), br.split_array(vec, n << w, w, parents, outcomes, qubit, release))
                big.branch_split(src, w, parents[:999], outcomes[:999], qubit, release)
                assert bits_equal(big.amplitudes(), br.split_array(vec, 2 * n << w, w, parents[:999], outcomes[:999], qubit, release))
        assert bits_equal(src.amplitudes(), vec)


@pytest.mark.parametrize("w", WIDTHS + [16])
def test_mass_order_contract(lib, w):
    """the same slot contents give the same bits at slot 0 of W = w, at slot 5 of W = w + 3 and at the last slot of
    W = w + 6, and with n_slots = 1 or all"""
    slot = rand_slots(w, 1, 300 + w)
    mid = rand_slots(w, 8, 301 + w)
    mid[5 << w: 6 << w] = slot
    mid[0: 1 << w] = slot
    top = rand_slots(w, 64, 302 + w, zero=(1, 62))
    top[63 << w:] = slot
    with lib.Engine(w) as a, lib.Engine(w + 3) as b, lib.Engine(w + 6) as c:
        a.set_amplitudes(0, slot)
        b.set_amplitudes(0, mid)
        c.set_amplitudes(0, top)
        for qubit in qubits_of(w):
            ma = a.branch_mass(w, 1, qubit)
            mb = b.branch_mass(w, 8, qubit)
            mc = c.branch_mass(w, 64, qubit)
            assert bits_equal(ma[0], mb[5]) and bits_equal(ma[0], mb[0]) and bits_equal(ma[0], mc[63]), (w, qubit)
            assert bits_equal(b.branch_mass(w, 1, qubit)[0], ma[0]) and bits_equal(b.branch_mass(w, 6, qubit), mb[:6])
            check_mass(mc, top, w, 64, qubit)


def test_mass_folded_by_a_workgroup(lib):
    """w = 23: the run sums of a slot are folded by a whole workgroup (one wave below that width)"""
    w = 23
    vec = rand_slots(w, 2, 9)
    with lib.Engine(w + 1) as e, lib.Engine(w) as one:
        e.set_amplitudes(0, vec)
        one.set_amplitudes(0, vec[1 << w:])
        for qubit in (0, 7, 11, w - 1):
            got = e.branch_mass(w, 2, qubit)
            check_mass(got, vec, w, 2, qubit)
            assert bits_equal(one.branch_mass(w, 1, qubit)[0], got[1])


def test_split_has_read_the_source_before_the_source_moves_on(lib):
    """the split runs on the destination's stream and the source's stream waits for it: a source overwritten at once
    does not reach the destination (the size of test_copy_state_has_read_the_source_before_the_source_moves_on)"""
    n, w = 26, 24
    with lib.Engine(n) as a, lib.Engine(n) as b:
        a.init_uniform((1 << n) - 1)
        a.apply_diag([0, n - 1], np.exp(1j * np.arange(4)))
        a.sync()
        src = a.amplitudes()
        parents, outcomes = [3, 0, 2, 1], [1, 0, 0, 1]
        want = br.split_array(src, 1 << n, w, parents, outcomes, w - 1, 1)
        for rep in range(2):
            b.branch_split(a, w, parents, outcomes, w - 1, 1)
            a.init_zero()                                     # overwrites the whole source at once
            assert bits_equal(b.amplitudes(), want), rep
            a.set_amplitudes(0, src)


def test_hidden_state_of_the_source(lib):
    """a source left by a folded init + diagonal program: implied zeros (the zero qubit above the slots, and inside them),
    and a deferred state (forced at 16 qubits by the engine option) -- sums and split as of the same amplitudes set plainly"""
    from _deferred_cases import BLOCK_BIT, REG_BIT, THREAD_BIT, W, default_ops, start
    w = 13
    OPTS = {"init_prod_r": 4, "init_prod_bit0": -1}      # the tile shape of test_gpu_deferred_state.test_implied_zeros
    parents, outcomes = [7, 1, 1, 4, 0], [1, 1, 0, 0, 1]
    for zq in (REG_BIT, THREAD_BIT, BLOCK_BIT):
        ops = default_ops(seed=80 + zq, zero=(zq,))
        twin = start(ops, 0, **OPTS)
        amps = twin.amplitudes()
        twin.close()
        with lib.Engine(W) as plain, lib.Engine(W) as dst:
            plain.set_amplitudes(0, amps)
            for defer in (0, 1):
                for qubit in (0, THREAD_BIT, BLOCK_BIT, w - 1):
                    hidden = start(ops, defer, **OPTS)
                    try:
                        assert hidden.state_info()["deferred"] == bool(defer)
                        assert bits_equal(hidden.branch_mass(w, 8, qubit), plain.branch_mass(w, 8, qubit))
                        assert not hidden.state_info()["deferred"]
                    finally:
                        hidden.close()
                    hidden = start(ops, defer, **OPTS)
                    try:
                        dst.branch_split(hidden, w, parents, outcomes, qubit, 1)
                        assert not hidden.state_info()["deferred"] and not dst.state_info()["deferred"]
                        assert bits_equal(dst.amplitudes(), br.split_array(amps, 1 << W, w, parents, outcomes, qubit, 1))
                        assert bits_equal(hidden.amplitudes(), amps)
                    finally:
                        hidden.close()
            # a destination that was deferred itself is a plainly stored state afterwards
            hidden = start(ops, 1, **OPTS)
            try:
                hidden.branch_split(plain, w, parents, outcomes, 2, 0)
                assert not hidden.state_info()["deferred"]
                want = br.split_array(amps, 1 << W, w, parents, outcomes, 2, 0)
                assert bits_equal(hidden.amplitudes(), want)
                check_mass(hidden.branch_mass(w, 5, 2), want, w, 5, 2)
                assert abs(hidden.norm() - float((np.abs(want) ** 2).sum())) < 1e-12
            finally:
                hidden.close()


def test_offsets_beyond_32_bits(lib):
    """Engine(33), 128 GiB, 8192 slots of w = 20 with only the last one populated: slot offsets need 64 bits"""
    free, _ = lib.device_memory(0)
    if free < 140 * 2 ** 30:
        pytest.skip("needs 140 GiB of free device memory, %.0f GiB are free" % (free / 2 ** 30))
    W, w = 33, 20
    n = 1 << (W - w)
    slot = rand_slots(w, 1, 44)
    with lib.Engine(W) as big, lib.Engine(w) as small:
        big.init_zero()
        big.set_amplitudes(0, np.zeros(1))                   # not even |0..0>: slot 0 is empty too
        big.set_amplitudes((n - 1) << w, slot)
        got = big.branch_mass(w, n, 7)
        assert (got[: n - 1] == 0).all()
        check_mass(got[n - 1:], slot, w, 1, 7)
        small.set_amplitudes(0, slot)
        assert bits_equal(small.branch_mass(w, 1, 7)[0], got[n - 1])
        small.init_zero()
        small.branch_split(big, w, [n - 1], [1], 7, 0)
        assert bits_equal(small.amplitudes(), br.split_array(slot, 1 << w, w, [0], [1], 7, 0))


def test_refusals(lib):
    with lib.Engine(6, devices=(0, 0)) as two, lib.Engine(6) as a, lib.Engine(6) as b:
        a.init_uniform(63)
        with pytest.raises(ValueError, match="shard"):
            two.branch_mass(3, 1, 0)
        with pytest.raises(ValueError, match="shard"):
            two.branch_split(a, 3, [0], [0], 0, 0)
        with pytest.raises(ValueError, match="shard"):
            a.branch_split(two, 3, [0], [0], 0, 0)
        with pytest.raises(ValueError, match="qubit"):
            a.branch_mass(3, 1, 3)
        with pytest.raises(ValueError, match="qubit"):
            b.branch_split(a, 3, [0], [0], 3, 0)
        with pytest.raises(ValueError, match="slots"):
            a.branch_mass(3, 9, 0)
        with pytest.raises(ValueError, match="slots"):
            a.branch_mass(3, 0, 0)
        with pytest.raises(ValueError, match="children"):
            b.branch_split(a, 3, [0] * 9, [0] * 9, 0, 0)
        with pytest.raises(ValueError, match="parent"):
            b.branch_split(a, 3, [8], [0], 0, 0)
        with pytest.raises(ValueError, match="outcome"):
            b.branch_split(a, 3, [0], [2], 0, 0)
        with pytest.raises(ValueError, match="same handle"):
            a.branch_split(a, 3, [0], [0], 0, 0)
        with pytest.raises(ValueError, match="slot width"):
            a.branch_mass(7, 1, 0)
        assert abs(a.norm() - 1.0) < 1e-12                    # nothing was touched
