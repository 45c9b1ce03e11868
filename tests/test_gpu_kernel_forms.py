"""GPU parity of the one-gate kernels in the forms that only large states or engine options select, against the numpy
oracle (oracle/sv_numpy.py): later iterations of the grid-stride loops, the unroll and pair_variant forms, marginals on
both sides of their LDS / global / temporary-scratch switches, and the direct gate entries on several virtual shards.

Why 22 qubits for the grid-stride tests.  grid_for (qsv.hip) caps a grid at n_cu * blocks_per_cu workgroups; with the
default 65536 per CU no state a test can hold reaches the cap, so ``base += stride`` never runs twice -- while a 34-qubit
shard needs 2^24 workgroups, one more than grid_for's absolute cap, and loops.  With blocks_per_cu = 1 the grid is n_cu
workgroups, and one iteration of a U = 4 kernel (256 threads x 4) covers n_cu * 1024 work items: 2^18 on the 256 CUs of
an MI355X, 2^19 on a device of 512.  A 22-qubit shard has 2^21 pairs; a gate with c controls leaves 2^(21 - c) of them.
Every gate of the stride tests has at most 2 controls, so every launch has at least 2^19 work items: two iterations or
more on any device of up to 512 CUs (eight uncontrolled on an MI355X).  The dense k-qubit kernel k_kq runs one thread
per group of 2^k amplitudes: k = 5 leaves 2^17 groups = two iterations of n_cu * 256 threads on 256 CUs, so k <= 5.

The grid size decides which workgroup handles an amplitude, never the arithmetic it gets: the same sequence with
blocks_per_cu = 1 and with the default must leave bit-identical states (np.array_equal) on top of the numpy tolerance.
Another unroll, nontemporal or pair_variant is another template instantiation: those are compared with numpy only.

Tolerances are those of tests/test_gpu_kernels.py: 1e-13 absolute on the amplitudes of a unit vector, 1e-12 where dense
k-qubit gates are in the sequence."""
import numpy as np
import pytest

from _kernel_forms import apply_engine, marginal, rand_mats, rand_state, rand_table, rand_u, reference, run_engine, run_numpy

pytestmark = pytest.mark.gpu
TOL = 1e-13
N = 22                                              # the grid-stride tests: see the module docstring
NT_SWZ = [(0, 0), (1, 2)]


@pytest.fixture(scope="module")
def lib():
    from qcmrf_amd import _lib
    _lib.load()
    assert _lib.device_count() >= 1
    return _lib


def access(nt, swz):
    return [("nontemporal", nt), ("multi_nt", nt), ("swizzle", swz)]


def check_stride(lib, key, seed, make_gates, options, tol=TOL, exact=False):
    """``make_gates()`` on N qubits with one workgroup per CU against numpy, and bit for bit against the default grid"""
    state, gates, ref = reference(key, N, seed, make_gates)
    capped = run_engine(lib, N, state, gates, options + [("blocks_per_cu", 1)])
    err = np.abs(capped - ref).max()
    print("%s %s: max |got - ref| = %.3g" % (key, options, err))
    assert err < tol
    if exact:
        assert np.array_equal(capped, ref)
    whole = run_engine(lib, N, state, gates, options)
    assert np.array_equal(capped, whole)


def controlled(cases, seed):
    """every (controls, target) as a controlled 2x2 and as an MCX, control values drawn per gate (both occur)"""
    rs = np.random.RandomState(seed)
    gates = []
    for i, (cs, t) in enumerate(cases):
        vals = [int(x) for x in rs.randint(0, 2, size=len(cs))]
        gates.append(("u", t, rand_u(1, seed + i), cs, vals))
        vals = [1 - v for v in vals] if i % 2 else vals
        gates.append(("x", cs, t, vals))
    return gates


# ------------------------------------------------------------------------------------------------------------------
# A. grid-stride loops: blocks_per_cu = 1 at 22 qubits
# ------------------------------------------------------------------------------------------------------------------
def gates_uncontrolled():
    gates = []
    for t in (0, 3, 4, 5, 6, 10, 11, 12, 21):
        gates.append(("u", t, rand_u(1, 200 + t), [], []))
        gates.append(("x", [], t, []))
    return gates


@pytest.mark.parametrize("shuffle", [1, 0])
@pytest.mark.parametrize("nt,swz", NT_SWZ)
def test_stride_uncontrolled_2x2_and_x(lib, nt, swz, shuffle):
    """dense 2x2 and X without controls: targets below bit 5 (and bit 5 without the swizzle) through the wave-shuffle
    sweep k_lowt, the others -- all of them with lowt_shuffle = 0 -- through k_pair, both in a loop of several iterations"""
    check_stride(lib, "uncontrolled", 61, gates_uncontrolled, access(nt, swz) + [("lowt_shuffle", shuffle)])


LOW_CTRL = [([1], 12), ([2], 0), ([0, 2], 1), ([0, 1], 21), ([1, 2], 4), ([0], 5), ([2], 11), ([1], 2), ([0, 2], 6), ([2], 1)]


@pytest.mark.parametrize("unroll", [4, 2, 1])
@pytest.mark.parametrize("mask", [1, 0])
@pytest.mark.parametrize("nt,swz", NT_SWZ)
def test_stride_controls_inside_a_cache_line(lib, nt, swz, mask, unroll):
    """1-2 controls on address bits 0..2, targets below, between and above them: the masked full-line sweep k_pair_m
    (lowctl_mask = 1, one tile per workgroup whatever the cap) and the enumerating k_pair (0), which loops"""
    check_stride(lib, "lowctl", 62, lambda: controlled(LOW_CTRL, 300), access(nt, swz) + [("lowctl_mask", mask), ("unroll", unroll)])


HIGH_CTRL = [([5], 11), ([11], 5), ([5, 11], 3), ([5, 11], 8), ([5, 11], 20), ([21], 0), ([21], 11), ([5, 21], 12),
             ([11, 21], 6), ([5], 0), ([11], 21), ([21, 11], 5)]


@pytest.mark.parametrize("unroll", [4, 2, 1])
@pytest.mark.parametrize("nt,swz", NT_SWZ)
def test_stride_controls_on_bits_5_11_and_the_top_bit(lib, nt, swz, unroll):
    """controls on the two bits the index swizzle exchanges and on the top bit, targets below, between and above: k_pair
    with U = 4, 2 and the guarded U = 1, the swizzled index formed anew in every iteration"""
    check_stride(lib, "highctl", 63, lambda: controlled(HIGH_CTRL, 400), access(nt, swz) + [("unroll", unroll)])


def gates_phase_diag():
    rs = np.random.RandomState(64)
    gates = []
    for qs in ([0], [5], [11], [21], [5, 11], [0, 21], [2, 12], [11, 21]):
        gates.append(("ph", qs, float(rs.uniform(-3, 3)), [int(x) for x in rs.randint(0, 2, size=len(qs))]))
    rest = [q for q in range(N) if q not in (5, 11, 21)]
    for k in (3, 11, 12, 13):                      # LDS tables (k <= 11) and tables read from global memory
        qs = [5, 11, 21] + [int(x) for x in rs.permutation(rest)[:k - 3]]
        qs = [qs[i] for i in rs.permutation(k)]
        gates.append(("diag", qs, rand_table(k, 500 + k)))
    return gates


@pytest.mark.parametrize("nt,swz", NT_SWZ)
def test_stride_mcphase_and_diag(lib, nt, swz):
    check_stride(lib, "phase_diag", 65, gates_phase_diag, access(nt, swz))


def gates_mux():
    rs = np.random.RandomState(66)
    gates = []
    for k in (0, 2, 5):
        for t in (0, 5, 11, 21):
            pool = [q for q in (5, 11, 21, 1, 7, 13, 20) if q != t]
            sel = pool[:2] if k == 2 else pool[:k]
            sel = [sel[i] for i in rs.permutation(len(sel))]
            gates.append(("mux", sel, t, rand_mats(k, 600 + 40 * k + t)))
    return gates


@pytest.mark.parametrize("unroll", [4, 2, 1])
@pytest.mark.parametrize("nt,swz", NT_SWZ)
def test_stride_mux(lib, nt, swz, unroll):
    """uniformly controlled 2x2 with 0, 2 and 5 selects (bits 5, 11 and the top bit among them) on targets 0, 5, 11, 21:
    k_mux<4> and, below unroll 4, k_mux<2>"""
    check_stride(lib, "mux", 67, gates_mux, access(nt, swz) + [("unroll", unroll)])


def gates_kq():
    rs = np.random.RandomState(68)
    gates = []
    for k, fixed in ((1, [21]), (2, [5, 11]), (3, [0, 11, 21]), (4, []), (5, [21, 5]), (5, [])):
        rest = [q for q in range(N) if q not in fixed]
        qs = fixed + [int(x) for x in rs.permutation(rest)[:k - len(fixed)]]
        gates.append(("kq", qs, rand_u(k, 700 + k)))
    return gates


@pytest.mark.parametrize("nt,swz", NT_SWZ)
def test_stride_dense_kq_on_the_vector_units(lib, nt, swz):
    """k_kq for k = 1..5 (kq_mfma = 0; kq3_tile = 0 keeps k = 3 there too): 2^17 groups at k = 5, two iterations"""
    check_stride(lib, "kq", 69, gates_kq, access(nt, swz) + [("kq_mfma", 0), ("kq3_tile", 0)], tol=1e-12)


@pytest.mark.parametrize("nt,swz", NT_SWZ)
def test_stride_swap_layout_local(lib, nt, swz):
    """k_swap_bits on the pairs (0, 21), (5, 11), (3, 12): a permutation, so exactly the host's"""
    check_stride(lib, "swap", 70, lambda: [("swap", 0, 21), ("swap", 5, 11), ("swap", 3, 12)], access(nt, swz), exact=True)


# ------------------------------------------------------------------------------------------------------------------
# B. forms that only an option selects, at the sizes that select them
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", range(1, 10))
def test_pair_variant_forms(lib, variant):
    """k_pair_x (pair_variant 1..9: separate non-temporal hints, U = 2 / 4 / 8, the XCD block remap) takes dense 2x2 gates
    whose pair count is a multiple of 16384: 16 qubits with 0 and 1 controls (2^15, 2^14 pairs), 17 qubits with 2"""
    rs = np.random.RandomState(variant)
    for n, cases in ((16, [([], 5), ([], 6), ([], 11), ([], 15), ([7], 5), ([5], 6), ([15], 11), ([3], 15), ([11], 15), ([12], 6)]),
                     (17, [([4, 9], 5), ([5, 16], 6), ([3, 12], 11), ([11, 16], 15), ([6, 14], 16)])):
        state = rand_state(n, 80 + n)
        gates = []
        for i, (cs, t) in enumerate(cases):
            gates.append(("u", t, rand_u(1, 800 + i), cs, [int(x) for x in rs.randint(0, 2, size=len(cs))]))
        ref = run_numpy(state, gates)
        got = run_engine(lib, n, state, gates, [("pair_variant", variant)])
        err = np.abs(got - ref).max()
        print("pair_variant %d, %d qubits: %.3g" % (variant, n, err))
        assert err < TOL, (variant, n)


@pytest.mark.parametrize("nt", [0, 1])
@pytest.mark.parametrize("unroll", [2, 1])
def test_unroll_forms_at_a_size_that_takes_four(lib, unroll, nt):
    """at 14 qubits every sweep divides by 1024 and runs with U = 4; unroll = 2 and 1 are the only way to k_pair<., 2>, to
    the guarded k_pair<., 1> with 1024 pairs or more, and to k_mux<2>: controlled 2x2, MCX and mux on targets 0, 5, 11, 13"""
    n = 14
    rs = np.random.RandomState(90)
    state = rand_state(n, 91)
    gates = controlled([([3], 0), ([9, 4], 5), ([5], 11), ([11, 12], 13), ([13], 0), ([6, 8], 11), ([12], 5), ([4], 13)], 900)
    for t in (0, 5, 11, 13):
        for k in (0, 3):
            sel = [int(x) for x in rs.permutation([q for q in range(n) if q != t])[:k]]
            gates.append(("mux", sel, t, rand_mats(k, 950 + 10 * t + k)))
    ref = run_numpy(state, gates)
    got = run_engine(lib, n, state, gates, [("unroll", unroll), ("nontemporal", nt), ("multi_nt", nt)])
    assert np.abs(got - ref).max() < TOL


# ------------------------------------------------------------------------------------------------------------------
# C. marginals: Engine.probabilities against np.bincount over |ref|^2
# ------------------------------------------------------------------------------------------------------------------
EPS = np.finfo(np.float64).eps


def check_single_terms(got, want):
    """entries that are ONE |amp|^2 each: the kernel's fma(re, re, im * im) against re * re + im * im, 2 ulp + numpy's own"""
    assert np.all(np.abs(got - want) <= 4 * EPS * want)


@pytest.fixture(scope="module")
def state16():
    ref = rand_state(16, 101)
    ref.setflags(write=False)
    return ref


@pytest.mark.parametrize("P", [1, 4])
def test_marginal_widths_across_the_lds_switch(lib, state16, P):
    """k = 0, 1, 11, 12 (pre-reduced in LDS), 13 and 16 (atomics straight to global memory), qubits in random order, on one
    shard and on four (the shards' partial tables added on the host)"""
    n = 16
    p = state16.real ** 2 + state16.imag ** 2
    rs = np.random.RandomState(102)
    with lib.Engine(n, devices=(0,) * P) as e:
        e.set_amplitudes(0, state16)
        for k in (0, 1, 11, 12, 13, 16):
            qs = [int(x) for x in rs.permutation(n)[:k]]
            got = e.probabilities(qs)
            want = marginal(p, qs)
            assert got.shape == want.shape
            if k == n:
                check_single_terms(got, want)
            else:
                assert np.abs(got - want).max() < TOL, k


def test_marginal_over_shard_bits_and_conditioned_on_them(lib, state16):
    """four shards (shard bits 14, 15): tables over both shard bits, one, none; conditioning on local bits only, on shard
    bits only -- with a fix_val that leaves whole shards out --, on both"""
    n = 16
    p = state16.real ** 2 + state16.imag ** 2
    lists = ([15, 14], [14, 15, 3], [7, 15, 0, 14, 11], [15], [2, 14, 9], [14], [13, 0, 5], [6], [15, 14] + list(range(11)),
             list(range(15, 1, -1)))
    masks = ((0, 0), ((1 << 3) | (1 << 11), 1 << 11), ((1 << 15) | (1 << 14), 1 << 15), (1 << 14, 0), (1 << 15, 1 << 15),
             ((1 << 15) | (1 << 14) | (1 << 0) | (1 << 9), (1 << 14) | (1 << 9)), ((1 << 14) | (1 << 13), (1 << 14) | (1 << 13)))
    with lib.Engine(n, devices=(0,) * 4) as e:
        e.set_amplitudes(0, state16)
        for qs in lists:
            for fm, fv in masks:
                got = e.probabilities(qs, fm, fv)
                assert np.abs(got - marginal(p, qs, fm, fv)).max() < TOL, (qs, fm, fv)


@pytest.mark.parametrize("P", [1, 4])
def test_marginal_structural_zeros_stay_exact_zeros(lib, P):
    """the kernel skips p == 0: an entry no amplitude contributes to comes back as exactly 0.0, LDS and global tables"""
    n = 16
    ref = rand_state(n, 103)
    ref[(np.arange(2 ** n) & 8) != 0] = 0
    ref /= np.linalg.norm(ref)
    p = ref.real ** 2 + ref.imag ** 2
    with lib.Engine(n, devices=(0,) * P) as e:
        e.set_amplitudes(0, ref)
        for qs in ([3], [9, 3, 15], [14, 3] + list(range(4, 14)), list(range(13)) + [15], list(range(n))[::-1]):
            got = e.probabilities(qs)
            want = marginal(p, qs)
            empty = ((np.arange(want.size) >> qs.index(3)) & 1) != 0
            assert np.all(got[empty] == 0.0) and np.all(want[empty] == 0.0), qs
            if len(qs) == n:
                check_single_terms(got, want)
            else:
                assert np.abs(got - want).max() < TOL, qs
        fm = (1 << 3) | (1 << 15)
        got = e.probabilities([1, 15], fm, fm)          # conditioned on the empty half: nothing at all
        assert np.all(got == 0.0)


def test_marginal_grid_stride(lib):
    """blocks_per_cu = 1 at 22 qubits: each thread of k_marginal walks 2^22 / (n_cu * 256) amplitudes (64 on 256 CUs)
    instead of 8 -- global (k = 13) and LDS (k = 3) tables, with and without a conditioning mask"""
    state = rand_state(N, 104)
    p = state.real ** 2 + state.imag ** 2
    with lib.Engine(N) as e:
        e.set_option("blocks_per_cu", 1)
        e.set_amplitudes(0, state)
        for qs in ([21, 0, 5, 11, 17, 3, 9, 12, 20, 1, 14, 7, 19], [11, 21, 5]):
            assert np.abs(e.probabilities(qs) - marginal(p, qs)).max() < TOL
        qs, fm, fv = [11, 21, 5], (1 << 20) | (1 << 2), 1 << 20
        assert np.abs(e.probabilities(qs, fm, fv) - marginal(p, qs, fm, fv)).max() < TOL


def test_marginal_wider_than_the_kept_scratch(lib):
    """k = 25 at 25 qubits: 2^25 table entries are more than the 2^24 doubles a shard keeps for reductions, so the call
    allocates and frees a buffer of its own -- twice, with a k = 3 marginal through the kept scratch in between.  Every
    entry is one |amp|^2; qubits (12..24, 5..11, 0..4) make the table a transposition of |ref|^2 as (2^13, 2^7, 2^5)"""
    n = 25
    rs = np.random.RandomState(105)
    w = rs.randn(32) + 1j * rs.randn(32)                     # 32 differently weighted copies of a 20-qubit state: cheap to make
    ref = (w[:, None] * rand_state(n - 5, 106)[None, :]).ravel()
    ref *= 1.0 / np.linalg.norm(ref)
    p = ref.real ** 2 + ref.imag ** 2
    qs = list(range(12, 25)) + list(range(5, 12)) + list(range(5))
    want = np.ascontiguousarray(p.reshape(1 << 13, 1 << 7, 1 << 5).transpose(2, 1, 0)).ravel()
    small = [24, 0, 11]
    want_small = p.reshape(2, 1 << 12, 2, 1 << 10, 2).sum(axis=(1, 3)).transpose(1, 2, 0).ravel()   # bit 0 <- 24, 1 <- 0, 2 <- 11
    with lib.Engine(n) as e:
        e.set_amplitudes(0, ref)
        first = e.probabilities(small)
        assert np.abs(first - want_small).max() < TOL
        check_single_terms(e.probabilities(qs), want)
        assert np.abs(e.probabilities(small) - want_small).max() < TOL
        check_single_terms(e.probabilities(qs), want)


# ------------------------------------------------------------------------------------------------------------------
# D. the direct gate entries on several virtual shards
# ------------------------------------------------------------------------------------------------------------------
def gates_on_shards(n, P):
    """gates whose controls / table qubits sit on shard bits, on local bits, on both; targets stay local"""
    g = P.bit_length() - 1
    L = n - g
    top = list(range(L, n))                          # the shard bits
    rs = np.random.RandomState(110 + P)
    gates = []
    # every control on a shard bit, both values: some shards are skipped, the others run an uncontrolled gate -- an X
    # through k_lowt (target < 5) or the pair sweep
    for vals in ([1] * g, [0] * g, [1] + [0] * (g - 1)):
        for t in (2, 0, 5, 9, L - 1):
            gates.append(("x", top, t, vals))
            gates.append(("u", t, rand_u(1, 1100 + t), top, vals))
    gates.append(("x", top[-1:], 3, [1]))
    gates.append(("u", 7, rand_u(1, 1120), top[-1:], [0]))
    # ... mixed with controls inside a 128-byte line and above
    for cs, t in ((top + [1], 6), ([0, top[0], 2], 4), ([top[-1], 2, 8], 1), ([5, top[0]], 11), ([1, 2] + top, 0)):
        vals = [int(x) for x in rs.randint(0, 2, size=len(cs))]
        gates.append(("x", cs, t, vals))
        gates.append(("u", t, rand_u(1, 1130 + t), cs, [1 - v for v in vals]))
    # phases: every qubit a shard bit (a scalar on the shards that match), one of several, none
    for qs in (top, top[:1], top + [4], [top[-1], 0, 11], [3, 10]):
        for vals in ([1] * len(qs), [int(x) for x in rs.randint(0, 2, size=len(qs))]):
            gates.append(("ph", qs, float(rs.uniform(-3, 3)), vals))
    # diagonals: all table qubits on shard bits (one entry per shard), some, none; k = 12, 13 and 14 with every shard bit
    # among them (sliced to 12 - g .. 14 - g local qubits: LDS up to 11, global memory beyond)
    lists = [top, top[::-1] + [6], [2, top[0]], [8, 1, 12 - g]]
    for k in (12, 13, 14):
        loc = [int(x) for x in rs.permutation(L)[:k - g]]
        qs = loc + top
        lists.append([qs[i] for i in rs.permutation(k)])
    for i, qs in enumerate(lists):
        gates.append(("diag", qs, rand_table(len(qs), 1200 + i)))
    # mux: selects all on shard bits (one matrix per shard), some, none; 10 selects, the most the entry takes
    loc = [int(x) for x in rs.permutation(np.arange(1, L))[:10 - g]]
    ten = loc + top
    for i, (sel, t) in enumerate(((top, 3), (top[::-1], 8), ([top[0], 2], 0), ([4, top[-1], 9], 5), ([1, 7], 11),
                                  ([ten[j] for j in rs.permutation(10)], 0), ([], L - 1))):
        gates.append(("mux", sel, t, rand_mats(len(sel), 1300 + 100 * i)))
    return gates


@pytest.mark.parametrize("P", [2, 4])
def test_direct_gate_entries_on_virtual_shards(lib, P):
    """qsv_apply_mc1q / mcx / mcphase / diag / mux_1q called directly on 2 and 4 virtual shards: resolve_gate evaluates the
    shard-bit controls per shard (skipping the shards that do not match) and slice_table cuts the tables down to the local
    qubits -- against sv_numpy on the whole vector"""
    n = 14
    state = rand_state(n, 111)
    gates = gates_on_shards(n, P)
    ref = run_numpy(state, gates)
    got = run_engine(lib, n, state, gates, devices=(0,) * P)
    assert np.abs(got - ref).max() < TOL


@pytest.mark.parametrize("P", [2, 4])
def test_direct_gate_entries_one_by_one_on_virtual_shards(lib, P):
    """the same gates one at a time, each from the same state: an error in one form is not averaged away by the next"""
    n = 14
    state = rand_state(n, 112)
    with lib.Engine(n, devices=(0,) * P) as e:
        for i, g in enumerate(gates_on_shards(n, P)):
            e.set_amplitudes(0, state)
            apply_engine(e, g)
            err = np.abs(e.amplitudes() - run_numpy(state, [g])).max()
            assert err < TOL, (i, g[0], g[1])


@pytest.mark.parametrize("P", [2, 4])
def test_direct_gate_entries_refuse_a_target_on_a_shard_bit(lib, P):
    n = 14
    state = rand_state(n, 113)
    with lib.Engine(n, devices=(0,) * P) as e:
        e.set_amplitudes(0, state)
        for t in range(e.local_qubits, n):
            with pytest.raises(RuntimeError):
                e.apply_1q(t, np.eye(2), [0], [1])
            with pytest.raises(RuntimeError):
                e.apply_mcx([1], t)
            with pytest.raises(RuntimeError):
                e.apply_mux([2, 3], t, rand_mats(2, 5))
            with pytest.raises(RuntimeError):
                e.apply_kq([0, t, 4], rand_u(3, 6))
        assert np.array_equal(e.amplitudes(), state)      # a refused gate has touched nothing
