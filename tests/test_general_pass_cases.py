"""The programs of tests/test_gpu_general_pass.py, checked on the CPU: the sharded numpy engine they are compared with
agrees with the dense gate-level oracle, each program holds the shapes and op counts its case claims, and losing any one
of the ops a case is about moves the state far beyond the tolerance of the GPU comparison."""
import numpy as np
import pytest

import _general_pass_cases as gp
from oracle.sharded_numpy import NumpyEngine
from qcmrf_amd import program


def small_cases():
    out = []
    for R in range(1, 6):
        out += [gp.shape_case(R, 14, True), gp.shape_case(R, 14, False), gp.shape_case(R, 10, False)]
    out += [gp.mask_case(N, pat) for N, pat in gp.MASK_CASES]
    out += [gp.mask_case(64, "half", P) for P in (2, 4)]
    out += [gp.cut_case(pm, N) for pm, N, _ in gp.CUT_CASES]
    for L in (14, 16):
        for zt in (0, 1):
            out += [gp.init_masked_case(L, zt), gp.init_h_case(L, zt)]
    out += [c for c, _ in gp.streak_cases()]
    return out


SMALL = small_cases()


def sharded(case, P, state=None):
    """the case's records through NumpyEngine on P shards (the case's own qubit count: its shard-bit controls then sit on
    local qubits for P = 1, which is the same operator)"""
    rec, data = program.encode(case.ops)
    ref = NumpyEngine(case.W, P)
    if state is not None:
        for s in range(P):
            ref.sh[s][:] = state[s << ref.L: (s + 1) << ref.L]
    ref.exec(rec, data)
    return ref.amplitudes()


@pytest.mark.parametrize("case", SMALL, ids=repr)
def test_numpy_engine_equals_the_dense_oracle_on_every_program(case):
    state = None if case.init else gp.rand_state(case.W, 11)
    want = gp.run_dense(case.ops, case.W, state)
    top = max(max(op.dense_targets(), default=0) for op in case.ops)
    for P in (1, 2, 4):
        if top >= case.W - (P.bit_length() - 1):
            continue                                          # a dense target on a shard bit: not a program of P shards
        assert np.abs(sharded(case, P, state) - want).max() < 1e-13, P


def test_numpy_engine_equals_the_dense_oracle_at_19_qubits():
    case = gp.many_block_bits_case()
    state = gp.rand_state(case.W, 11)
    want = gp.run_dense(case.ops, case.W, state)
    for P in (1, 2, 4):
        assert np.abs(sharded(case, P, state) - want).max() < 1e-13, P


@pytest.mark.parametrize("P", [2, 4])
def test_shard_fold_program_on_one_shard_equals_the_dense_oracle(P):
    case = gp.shard_fold_case(P)
    assert np.abs(sharded(case, 1) - gp.run_dense(case.ops, case.W)).max() < 1e-13


@pytest.mark.parametrize("R", [1, 2, 3, 4, 5])
def test_shape_programs_hold_every_shape_on_every_target(R):
    for L, lane in ((14, True), (14, False), (10, False)):
        case = gp.shape_case(R, L, lane)
        for xframe in (True, False):
            p = gp.plan(case.ops, L, lane_mode=case.lane_mode, xframe=xframe)
            assert p["R"] == R and p["ops"] + p["framed"] == len(case.ops)
            assert p["ops"] <= 112                            # one pass with pass_max_ops = 200
            for s in gp.SHAPES:
                assert (p["hist"][s] > 0) == (s in case.must_show), (L, lane, s)
        assert len(case.must_show) == (11 if lane else 7) - (R == 1)
        assert (min(p["reg"]) < 6) == (not lane)              # lane mode off: register offsets reach address bits 0..5
        # every register target meets every shape a register target can have, every lane bit every lane shape
        reg = p["reg"]
        seen = dict((t, set()) for t in reg + (list(range(6)) if lane else []))
        ctl = dict((t, set()) for t in reg)
        lanes, waves, blocks = gp.bit_classes(L, reg)
        for op in case.ops:
            kind, t, qs = gp.local_op(op, L, 0)
            shape = gp.shape_of((kind, t, qs), reg, case.lane_mode)
            if kind == "mcphase":
                t, qs = qs[0], qs[1:]
            if t >= 0:
                seen[t].add(shape)
            for q in (qs if kind == "diag" else ()):          # a diagonal has no target: it counts for the register bits it reads
                if q in reg:
                    seen[q].add(shape)
            if kind in ("u", "x", "mcphase") and t in ctl:
                cls = tuple(sorted("reg" if q in reg else "lane" if q in lanes else "wave" if q in waves else "block" for q in qs))
                vals = tuple(op.vals[-len(qs):]) if qs else ()
                ctl[t].add((cls, vals))
        for t in reg:
            assert {"x", "mat", "phase", "tab_t", "diag_a"} <= seen[t]
            assert R == 1 or "tab_p" in seen[t]
            places = set(c for c, _ in ctl[t])
            assert () in places
            if L == 14:
                want = {("lane",), ("wave",), ("block",)} | ({("reg",), ("block", "reg")} if R > 1 else set())
                assert want <= places, (t, places)
                for c in want:                                # both control values
                    assert len(set(v for cc, v in ctl[t] if cc == c)) >= 2, (t, c)
        for l in (range(6) if lane else ()):
            assert {"ltab_t", "ltab_a", "lx", "lmat"} <= seen[l]


def test_mask_programs_own_the_mask_words_they_claim():
    M = 2 ** 64 - 1
    for N, pat in gp.MASK_CASES:
        case = gp.mask_case(N, pat)
        bits, words = gp.owned_words(case)
        p = gp.plan(case.ops, case.L)
        assert p["R"] == 4 and p["ops"] == N and all(p["hist"][s] > 0 for s in ("x", "mat", "phase"))
        if pat == "half":
            assert bits == [15] and words[(1,)] == (0x00000000FFFFFFFF, 0) and words[(0,)] == (0xFFFFFFFF00000000, 0)
        else:
            assert bits == [14, 15]
            assert words[(1, 1)] == ((1 << pat) & M, (1 << pat) >> 64)
    assert sorted(set(N for N, _ in gp.MASK_CASES)) == [32, 33, 64, 65, 96, 126]
    assert set(p for _, p in gp.MASK_CASES) == {"half", 31, 63, 64, 95, 125}
    # virtual shards: the op lists, hence the words, differ from shard to shard
    for P in (2, 4):
        case = gp.mask_case(64, "half", P)
        lists = [gp.owned_words(case, s)[1] for s in range(P)]
        assert len(set(gp.plan(case.ops, case.L, s)["ops"] for s in range(P))) >= 2
        assert all(gp.plan(case.ops, case.L, s)["ops"] >= 2 for s in range(P))
        assert lists[P // 2] == {(1,): (0x00000000FFFFFFFF, 0), (0,): (0xFFFFFFFF00000000, 0)}
        assert lists[0] != lists[P // 2]


def test_ten_block_bits_leave_two_to_the_exec_mask():
    case = gp.many_block_bits_case()
    kept, left = gp.combo_bits(case)
    p = gp.plan(case.ops, case.L)
    assert p["R"] == 1 and p["ops"] == len(case.ops) <= 64
    assert len(kept) == 8 and len(left) == 2 and len(case.sentinels) >= 2
    assert all(p["hist"][s] > 0 for s in case.must_show)


def test_cut_programs_have_the_lengths_the_rule_is_about():
    for pm, N, passes in gp.CUT_CASES:
        case = gp.cut_case(pm, N)
        assert gp.plan(case.ops, case.L)["ops"] == N == sum(passes)
        cap = min(56 if pm is None else pm, 112)              # the engine's default is 56
        assert passes[0] == (N if N - cap <= cap // 8 else cap)


def test_init_programs_hold_what_they_claim():
    for L in (14, 16):
        for zt in (0, 1):
            case = gp.init_masked_case(L, zt)
            mask = case.ops[0].mask
            p = gp.plan(case.ops[1:], L, lane_mode=case.lane_mode, xframe=False)
            assert p["R"] == case.options["multi_r"] == (4 if zt else 3)
            assert all(p["hist"][s] > 0 for s in case.must_show)
            lanes, waves, blocks = gp.bit_classes(L, [6, 7, 8])
            for cls in ([6, 7, 8], lanes, waves, blocks):     # the mask leaves out a bit of every class, and not all of any
                assert 0 < sum(1 for b in cls if not (mask >> b) & 1) < len(cls)
            assert not (mask >> 3) & 1 and case.ops[1].target == 3 and case.ops[2].target == 7
            case = gp.init_h_case(L, zt)
            p = gp.plan(case.ops[1:], L, lane_mode=case.lane_mode, xframe=False)
            assert p["R"] == case.options["multi_r"] == (5 if zt else 3) and p["hist"]["mat"] + p["hist"]["lmat"] >= 5
            p = gp.plan(case.ops[6:], L, lane_mode=case.lane_mode, xframe=False)
            assert p["R"] == case.options["multi_r"] and p["ops"] == len(case.ops) - 6


def sensitivity(case, state):
    full = gp.run_dense(case.ops, case.W, state)
    return [float(np.abs(gp.run_dense(case.ops, case.W, state, skip=k) - full).max()) for k in case.sentinels]


@pytest.mark.parametrize("case", [gp.mask_case(N, pat) for N, pat in gp.MASK_CASES] + [gp.many_block_bits_case()] +
                         [gp.shape_case(R, 14, True) for R in range(1, 6)], ids=repr)
def test_dropping_a_sentinel_op_moves_the_state(case):
    """ops 31, 32, 63 of the half pattern, the single op a workgroup class owns (31, 63, 64, 95, 125), the ops left to the
    exec-mask test, one op per shape: without it the state differs by at least 1e-6 (max-abs), a million times the
    tolerance of the GPU comparison"""
    assert case.sentinels
    moved = sensitivity(case, gp.rand_state(case.W, 11))
    assert min(moved) >= 1e-6, list(zip(case.sentinels, moved))


def test_sentinels_are_the_ops_the_issue_names():
    got = set()
    for N, pat in gp.MASK_CASES:
        got |= set(gp.mask_case(N, pat).sentinels)
    assert got == {31, 32, 63, 64, 95, 125}
    for R in range(1, 6):
        case = gp.shape_case(R, 14, True)
        p = gp.plan(case.ops, 14, xframe=False)
        shapes = set(gp.shape_of(gp.local_op(case.ops[k], 14, 0), p["reg"], True) for k in case.sentinels)
        assert shapes == set(case.must_show)
