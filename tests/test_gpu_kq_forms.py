"""GPU parity of the matrix-core dense-gate kernels (k_kq_mfma, k_kq_mfma3 in its PF / ALDS forms, k_kq_mfma3w, k_kq_lds
with 1, 2, 3 batches of loads in flight, and k_kq_tile) against oracle.sv_numpy.apply_kq: every target set of a 14-qubit
shard under the default selection, every explicit variant on the placements its lane and instruction maps branch on, and
the walk shapes of tests/_kq_cases.py -- the shapes large shards take, reached here with the option kq_grid.

Gates are checked ONE BY ONE: after each gate the state is read back and compared with numpy applied to the state read
back before that gate (the first one is what set_amplitudes wrote).  Rounding does not accumulate over the thousands of
gates of a sweep, and a failure names its target set, in the order presented, with the variant and options that ran.
The bound per gate is the 1e-12 absolute of tests/test_gpu_kernels.py for these kernels.

Why 14 qubits.  launch_kq_mfma builds the map of k_kq_lds from where the targets lie relative to address bits 3 (a target
inside a 128-byte line selects the kernel), 5 (the sixth lane bit) and 11 (the bit that lane bit takes when swizzle is on:
swizzle 2 from L = 14, swizzle 1 -- the default -- from L = 26 by the same code).  L = 14 is the smallest shard with the
exchange, and its 14 address bits lie on both sides of all three.

Which workgroup or wave computes a batch must not change a bit of it: rows with a grid cap are also compared with
np.array_equal against the same gate from the same state without the cap."""
from itertools import combinations

import numpy as np
import pytest

import _kq_cases as kc
from _kernel_forms import rand_state, rand_u
from oracle import sv_numpy as sv

pytestmark = pytest.mark.gpu
TOL = 1e-12
L14 = 14
ACCESS = [(2, 0), (2, 1), (0, 0)]                    # (swizzle, nontemporal)


@pytest.fixture(scope="module")
def lib():
    from qcmrf_amd import _lib
    _lib.load()
    assert _lib.device_count() >= 1
    return _lib


class Tally:
    """gates run and the worst per-gate error of one test function"""

    def __init__(self, name):
        self.name, self.gates, self.worst = name, 0, 0.0

    def report(self):
        print("KQ forms %s: %d gates, worst per-gate max |got - numpy| = %.3g" % (self.name, self.gates, self.worst))


def set_options(e, options):
    for name, value in options:
        e.set_option(name, value)


def check_gate(e, prev, qs, u, what, tally):
    """one gate on the engine (which holds ``prev``) against numpy on ``prev``; returns the state read back"""
    e.apply_kq(qs, u)
    got = e.amplitudes()
    ref = sv.apply_kq(prev.copy(), qs, u)
    err = float(np.abs(got - ref).max())
    tally.gates += 1
    tally.worst = max(tally.worst, err) if err == err else float("nan")
    assert err < TOL, "%s, targets %s: max |got - numpy| = %.3g" % (what, list(qs), err)
    return got


def sweep(lib, n, options, sets, seed, name, devices=(0,)):
    """every target list of ``sets`` as one gate with a fresh random unitary, one by one on one engine"""
    tally = Tally(name)
    prev = rand_state(n, seed)
    with lib.Engine(n, devices=devices) as e:
        set_options(e, options)
        e.set_amplitudes(0, prev)
        try:
            for i, qs in enumerate(sets):
                prev = check_gate(e, prev, qs, rand_u(len(qs), 1000 * seed + i), "%s %s gate %d" % (name, options, i), tally)
        finally:
            tally.report()
    return tally


def presented(sets, seed):
    """each sorted target set in a seeded random order of its qubits -- the first set of every lowest target as it is
    (the identity order, where kq_order 0 and the K = 3 padding see ascending targets)"""
    rs = np.random.RandomState(seed)
    out, seen = [], set()
    for s in sets:
        s = sorted(s)
        if s[0] not in seen:
            seen.add(s[0])
            out.append(list(s))
        else:
            out.append([s[j] for j in rs.permutation(len(s))])
    return out


# ------------------------------------------------------------------------------------------------------------------
# a. every target set of a 14-qubit shard, the kernels chosen by K and placement
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("swz,nt", ACCESS)
@pytest.mark.parametrize("k", [3, 4, 5])
def test_every_target_set_default_selection(lib, k, swz, nt):
    """kq_variant -1: K = 4 (and K = 3 padded, kq3_tile 0) k_kq_lds<4> with a target below bit 3, k_kq_mfma3w<4> else;
    K = 5 k_kq_lds<5, PD = 3> with a target below bit 3, k_kq_mfma3<5, PF, ALDS> else -- all 364 / 1001 / 2002 sets"""
    sets = presented(combinations(range(L14), k), 140 + k)
    assert len(sets) == {3: 364, 4: 1001, 5: 2002}[k]
    options = [("kq3_tile", 0), ("swizzle", swz), ("nontemporal", nt)]
    sweep(lib, L14, options, sets, 10 * k + swz + nt, "a default k=%d" % k)


@pytest.mark.parametrize("swz,nt", ACCESS)
def test_every_target_set_k3_on_the_vector_units(lib, swz, nt):
    """kq3_tile 2: k_kq_tile<3> whatever the targets (its swizzle trades the sixth free address bit for bit 11)"""
    sets = presented(combinations(range(L14), 3), 143)
    assert len(sets) == 364
    options = [("kq3_tile", 2), ("swizzle", swz), ("nontemporal", nt)]
    sweep(lib, L14, options, sets, 33 + swz + nt, "a tile k=3")


# ------------------------------------------------------------------------------------------------------------------
# b. every explicit variant on the placements the maps branch on
# ------------------------------------------------------------------------------------------------------------------
def with_bit_11(k):
    return [s for s in combinations(range(L14), k) if 11 in s]


def structured_sets(k):
    """contiguous targets; every set with a target on bit 11; every lowest target 0..5 with the rest below 11, on both
    sides of 11, on the top bits; and -- the map of k_kq_lds gives lane bit 5 to bit 11 in exchange for a GROUP bit only when
    two targets lie below bit 5 and none on 5 or 11 -- every pair of targets below bit 6 with the rest below and above 11"""
    sets = {tuple(range(a, a + k)) for a in range(L14 - k + 1)}
    sets |= set(with_bit_11(k))
    rests = {4: ((7, 9, 10), (10, 12, 13), (11, 12, 13)), 5: ((7, 8, 9, 10), (9, 10, 12, 13), (10, 11, 12, 13))}[k]
    for low in range(6):
        sets |= {(low,) + rest for rest in rests}
    pair_rests = {4: ((8, 10), (12, 13)), 5: ((7, 8, 10), (10, 12, 13))}[k]
    for a, b in combinations(range(6), 2):
        sets |= {(a, b) + rest for rest in pair_rests}
    return sorted(sets)


@pytest.mark.parametrize("k", [4, 5])
@pytest.mark.parametrize("variant", range(9))
def test_every_variant_on_structured_target_sets(lib, variant, k):
    sets = presented(structured_sets(k), 200 + k)
    assert len(sets) == {4: 336, 5: 764}[k]
    options = [("kq_variant", variant), ("swizzle", 2), ("nontemporal", 0)]
    sweep(lib, L14, options, sets, 50 + 2 * variant + k, "b variant %d k=%d" % (variant, k))


@pytest.mark.parametrize("k", [4, 5])
@pytest.mark.parametrize("order", [0, 2, 3, 4])
@pytest.mark.parametrize("variant", [0, 3, 5, 8])
def test_target_orders_on_sets_with_bit_11(lib, variant, order, k):
    """kq_order decides which target is index bit 0, 1 of the re-indexed matrix, i.e. the lanes' part of a row offset in
    k_kq_mfma / k_kq_mfma3 (kq), k_kq_mfma3w (okh, o2) and the image offsets of k_kq_lds: one variant per kernel, every set
    with a target on bit 11 (the default order 1 moves exactly that target, and runs in every other test)"""
    sets = presented(with_bit_11(k), 300 + k)
    options = [("kq_variant", variant), ("kq_order", order), ("swizzle", 2), ("nontemporal", 0)]
    sweep(lib, L14, options, sets, 400 + 10 * variant + order + k, "b order %d variant %d k=%d" % (order, variant, k))


# ------------------------------------------------------------------------------------------------------------------
# c. walk shapes: the rows of _kq_cases.py
# ------------------------------------------------------------------------------------------------------------------
def three_sets(L, k, seed):
    """targets 0..k-1, a set with a target on bit 11 (where the shard has one), a seeded random set"""
    rs = np.random.RandomState(seed)
    sets = [list(range(k))]
    if L > 11:
        qs = [int(q) for q in rs.permutation(L)[:k]]
        if 11 not in qs:
            qs[int(rs.randint(k))] = 11
        sets.append(qs)
    sets.append([int(q) for q in rs.permutation(L)[:k]])
    return sets


def row_options(row):
    return [("kq3_tile", 0), ("kq_variant", row.variant), ("kq_chunked", row.chunked), ("nontemporal", row.nontemporal),
            ("swizzle", row.swizzle), ("kq_grid", row.kq_grid)]


def run_row(e, row, state, sets, tally, what):
    """the gates of ``sets`` from ``state`` under the row's options, one by one; a capped row also without its cap"""
    set_options(e, row_options(row))
    e.set_amplitudes(0, state)
    prev = state
    for i, qs in enumerate(sets):
        u = rand_u(len(qs), 7000 + 10 * row.L + i)
        got = check_gate(e, prev, qs, u, "%s %s" % (what, row), tally)
        if row.kq_grid:
            e.set_option("kq_grid", 0)
            e.set_amplitudes(0, prev)
            e.apply_kq(qs, u)
            free = e.amplitudes()
            e.set_option("kq_grid", row.kq_grid)
            assert np.array_equal(got, free), "%s %s, targets %s: kq_grid changes %d amplitudes" % (what, row, qs, int((got != free).sum()))
        prev = got


def walk_pieces():
    """the rows by (k, L); the 2 MiB states of L = 17 cost most to move, so their rows go three variants at a time"""
    pieces = []
    for k, L in sorted({(r.k, r.L) for r in kc.ROWS}):
        for lo in (0, 3, 6) if (L == 17 and k > 3) else (0,):
            pieces.append((k, L, lo, lo + 2 if (L == 17 and k > 3) else 8))
    return pieces


@pytest.mark.parametrize("k,L,v0,v1", walk_pieces())
def test_walk_shapes(lib, k, L, v0, v1):
    rows = [r for r in kc.ROWS if (r.k, r.L) == (k, L) and v0 <= r.variant <= v1]
    assert rows
    tally = Tally("c walks k=%d L=%d variants %d..%d (%d rows)" % (k, L, v0, v1, len(rows)))
    state = rand_state(L, 500 + L)
    sets = three_sets(L, k, 600 + 20 * k + L)
    with lib.Engine(L) as e:
        try:
            for row in rows:
                run_row(e, row, state, sets, tally, "c")
        finally:
            tally.report()


def test_blocks_per_cu_changes_no_bit(lib):
    """kq_blocks_per_cu = 1 at L = 16, K = 5 under the default selection (k_kq_lds on low targets, k_kq_mfma3 else)"""
    L, k = 16, 5
    tally = Tally("c kq_blocks_per_cu")
    state = rand_state(L, 516)
    sets = [[0, 1, 2, 3, 4], [5, 3, 14, 8, 11], [2, 15, 11, 9, 6]] + three_sets(L, k, 616)[2:]
    got = {}
    for bpc in (1, 0):
        with lib.Engine(L) as e:
            set_options(e, [("swizzle", 2), ("kq_blocks_per_cu", bpc)])
            e.set_amplitudes(0, state)
            prev, got[bpc] = state, []
            for i, qs in enumerate(sets):
                prev = check_gate(e, prev, qs, rand_u(k, 7100 + i), "c kq_blocks_per_cu %d" % bpc, tally)
                got[bpc].append(prev)
    tally.report()
    for a, b, qs in zip(got[1], got[0], sets):
        assert np.array_equal(a, b), qs


# ------------------------------------------------------------------------------------------------------------------
# d. virtual shards: the entry loops over them
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [12, 14])
@pytest.mark.parametrize("P", [2, 4])
def test_tail_of_two_rows_on_virtual_shards(lib, P, L):
    """k = 5 with k_kq_lds<5, PD = 3> (variant 8) at L = 12 and 14 local qubits: every wave has 2 and 8 batches, a tail of
    two -- on every one of P shards of one device"""
    row = [r for r in kc.ROWS if (r.L, r.k, r.variant, r.kq_grid) == (L, 5, 8, 0)][0]
    assert all(w.tail == 2 for w in kc.waves_of(row, 256)[1])
    n = L + P.bit_length() - 1
    tally = Tally("d P=%d L=%d" % (P, L))
    with lib.Engine(n, devices=(0,) * P) as e:
        assert e.local_qubits == L
        try:
            run_row(e, row._replace(swizzle=2), rand_state(n, 700 + n), three_sets(L, 5, 800 + n), tally, "d P=%d" % P)
        finally:
            tally.report()
