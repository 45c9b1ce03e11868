"""The programs of tests/test_gpu_table_pass.py, checked on the CPU: the host model of _table_pass_cases answers every case
consistently and with the pass structure the case is about, the sharded numpy engine the device is compared with agrees with
the dense gate-level oracle, and every sentinel holds -- losing an op, transposing one table entry (s0 <-> s1), exchanging
its diagonal (c0 <-> c1) or reversing an order-sensitive pair moves the state by more than 1e-6, a million times the tolerance
of the GPU comparison."""
import numpy as np
import pytest

import _general_pass_cases as gp
import _table_pass_cases as tp
from oracle.sharded_numpy import NumpyEngine
from qcmrf_amd import program

A_CASES = [tp.inst_case(R, mode, init, v) for v in tp.A_TARGETS for R in range(1, 7) for mode in (1, 2) for init in (False, True)]
B_CASES = ([tp.init_case(k) for k in tp.B_KINDS] + [tp.init_case("dead", 2, n) for n in (1, 2, 4, 5, 6)] +
           [tp.init_case("one-live", 2, 6), tp.init_case("dead", 1), tp.init_case("one-live", 1)])
C_CASES = [tp.pair_case(k, o) for k in tp.C_PAIRS for o in (0, 1)]
CHAINS = [tp.same_target_case()] + [tp.chain_case(N, pm) for pm, N, _ in tp.CHAIN_CUTS]
D_CASES = [tp.lane_case(s, P, 2, sel11) for s in tp.D_SHAPES for P in (1, 2, 4) for sel11 in (True, False)] + \
          [tp.final_x_case(False), tp.final_x_case(True)]
E_CASES = [tp.xframe_case(init, mode) for init in (False, True) for mode in (1, 2)]
F_CASES = [tp.budget_case(False), tp.budget_case(True)] + [tp.big_mux_case(k) for k in tp.F_BIG]
G_CASES = [tp.zero_case(1), tp.zero_case(2)]
ALL = A_CASES + B_CASES + C_CASES + CHAINS + D_CASES + E_CASES + F_CASES + G_CASES


def start(case):
    return None if case.init else gp.rand_state(case.W, 11)


def final(case, ops=None, skip=None):
    return gp.run_dense(case.ops if ops is None else ops, case.W, start(case), skip=skip)


def moved(case, ops=None, skip=None):
    return float(np.abs(final(case, ops, skip) - final(case)).max())


def test_case_names_are_unique():
    assert len(set(c.name for c in ALL)) == len(ALL)


@pytest.mark.parametrize("case", ALL, ids=repr)
def test_model_is_self_consistent(case):
    settings = tp.D_SETTINGS if case.name.startswith("lanes") else [{}]
    for st in settings:
        try:
            lines, launches, fused = tp.plan_case(case, **st)
        except tp.NotATablePass:
            assert case.name.endswith("sel11=1")      # lane_case_for takes the program without that select there
            continue
        for s in range(case.P):
            mine = [l for l in lines if l["shard"] == s]
            nx = sum(1 for op in case.ops if op.kind == "x")
            nops = sum(1 for op in case.ops if op.kind in ("mux", "diag"))
            in_pass = sorted(i for l in mine for i in l["members"])
            assert len(in_pass) == len(set(in_pass)) and all(case.ops[i].kind in ("mux", "diag") for i in in_pass)
            singles = sum(launches.get(k, 0) for k in ("mux", "diag")) // case.P
            assert len(in_pass) + singles + launches.get("init_prod", 0) == nops
            assert [i for l in mine for i in l["members"]] == in_pass          # program order across passes
        assert fused == sum(l["ops"] for l in lines) + case.P * nx
        assert launches.get("multi", 0) + launches.get("multi_init", 0) == len(lines)
        for l in lines:
            h = l["hist"]
            assert h["tab_t"] == l["rounds"] * l["R"] and h["diag_t"] + h["ltab_t"] + sum(1 for i in l["members"] if case.ops[i].target in l["reg"]) == l["ops"]
            assert all(h[s] == 0 for s in gp.SHAPES if s not in ("tab_t", "diag_t", "ltab_t"))
            assert 1 <= l["R"] <= 6 and l["tables"] <= 2560 and 1 <= l["rounds"] <= l["ops"] and l["ops"] <= 128
            assert sorted(i for r in l["round_lists"] for i in r) == sorted(i for i in l["members"] if case.ops[i].target not in l["reg"])
            assert (l["mode"] == 2) == all(case.ops[i].kind == "mux" and tp.is_rx(case.ops[i].mats) for i in l["members"])
            lanes, waves, blocks = l["classes"]
            assert len(set(lanes + waves + blocks + l["reg"])) == len(lanes + waves + blocks + l["reg"])
            if l["lanes"][0] >= 0:
                assert list(l["lanes"]) == lanes[3:6] and not set(l["lanes"]) & set(l["reg"])
        if case.mode is not None and not case.name.startswith(("budget", "big")):
            assert all(l["mode"] == case.mode for l in lines), case.name


@pytest.mark.parametrize("case", A_CASES + B_CASES + C_CASES + CHAINS[:2] + D_CASES[::6] + E_CASES + F_CASES[:2] + G_CASES, ids=repr)
def test_numpy_engine_equals_the_dense_oracle(case):
    want = final(case)
    rec, data = program.encode(case.ops)
    for P in sorted(set((1, case.P))):
        ref = NumpyEngine(case.W, P)
        st = start(case)
        if st is not None:
            for s in range(P):
                ref.sh[s][:] = st[s << ref.L: (s + 1) << ref.L]
        ref.exec(rec, data)
        assert np.abs(ref.amplitudes() - want).max() < 1e-13 * max(1.0, np.abs(want).max()), P
    assert 1e-3 < np.abs(want).max() < 1e3            # the non-unitary tables leave the state at a scale the tolerances are about


# ---------------------------------------------------------------------------------------------------------------------
# what each family claims
# ---------------------------------------------------------------------------------------------------------------------
def test_family_a_reaches_every_instantiation():
    seen = set()
    for case in A_CASES:
        lines, launches, _ = tp.plan_case(case)
        assert len(lines) == 1 and sum(launches.values()) == 1
        l = lines[0]
        assert (l["R"], l["mode"], l["init"]) == (case.R, case.mode, int(case.init))
        seen.add((l["R"], l["mode"], l["init"]))
        variant = case.name.split()[-1]
        assert l["reg"] == tp.A_TARGETS[variant][:case.R]
        assert l["nthreads"] == 2 ** (case.L - case.R)
        lanes, waves, blocks = l["classes"]
        muxes = [op for op in case.ops if op.kind == "mux"]
        for t in l["reg"]:
            ks = sorted(len(op.ctrls) for op in muxes if op.target == t)
            assert ks == [0, 1, 3]
        used = set(q for op in muxes for q in op.ctrls)
        assert used & set(lanes) and (not waves or used & set(waves)) and (not blocks or used & set(blocks))
        if variant == "lane14":
            assert sorted(op.target for op in muxes if op.target < 6) == list(range(6)) and l["hist"]["ltab_t"] == 6
        else:
            assert l["hist"]["ltab_t"] == 0 and l["lanes"] == (-1, -1, -1)
        if case.mode == 1:
            diags = [op.qubits for op in case.ops if op.kind == "diag"]
            assert sorted(len(q) for q in diags) == [1, 2, 3] and not set(q for d in diags for q in d) & set(l["reg"])
            assert variant != "lane14" or any(q < 6 for d in diags for q in d)
        if case.init:
            dead = all(not (case.ops[0].mask >> q) & 1 for q in l["reg"])
            assert dead == bool(case.R & 1)
    assert seen == set((R, m, i) for R in range(1, 7) for m in (1, 2) for i in (0, 1))
    small = dict((c.R, tp.plan_case(c)[0][0]["nthreads"]) for c in A_CASES if c.name.endswith("small10"))
    assert small[5] == 32 and small[6] == 16 and small[3] == 128          # workgroups of 256 threads that are partly empty


def test_family_b_takes_the_branches_it_names():
    for case in B_CASES:
        (l,), launches, _ = tp.plan_case(case)
        assert l["init"] == 1 and l["R"] == 5 and sorted(l["reg"]) == [6, 7, 8, 9, 10] and launches == {"multi_init": 1}
        mask = case.ops[0].mask
        all_dead = all(not (mask >> q) & 1 for q in l["reg"])
        kind = case.name.split()[1]
        assert all_dead == (kind in ("dead", "round1", "mask0"))
        if case.round0:
            assert l["round_lists"][0] == case.lane_ops and l["rounds"] == 1
        else:
            assert l["round_lists"][0] == [] and l["round_lists"][1] == case.lane_ops and l["rounds"] == 2
        lanes, waves, blocks = l["classes"]
        for i in case.lane_ops:
            sel = case.ops[i].ctrls
            assert sel[0] in waves and sel[1] in blocks
        if kind not in ("mask0", "full"):
            out = [q for q in range(case.L) if not (mask >> q) & 1]
            assert set(out) & set(lanes) and set(out) & set(waves) and set(out) & set(blocks)
    assert sorted(len(c.lane_ops) for c in B_CASES if c.name.startswith("init dead mode=2")) == [1, 2, 3, 4, 5, 6]


def test_family_c_pairs_cost_a_round_in_one_order():
    for kind in tp.C_PAIRS:
        r = [tp.plan_case(tp.pair_case(kind, o))[0][0] for o in (0, 1)]
        assert all(l["ops"] == 8 and l["R"] == 5 for l in r)
        if kind.startswith("gate"):
            assert r[0]["rounds"] == r[1]["rounds"] + 1      # the lane mux after the gate that reads its bit opens a round
        if kind == "gate-borrowed":
            assert r[0]["lanes"] == r[1]["lanes"] == (3, 4, 12)
    (l,), _, _ = tp.plan_case(tp.same_target_case())
    assert l["rounds"] == 40 and l["ops"] == 40
    for pm, N, passes in tp.CHAIN_CUTS:
        lines, launches, _ = tp.plan_case(tp.chain_case(N, pm))
        assert [x["ops"] for x in lines] == passes and launches == {"multi": len(passes)}


def test_family_d_lends_lanes_and_takes_the_map_where_it_says():
    plain = (-1, -1, -1)

    def lanes_of(shape, P=1, **st):
        return [l["lanes"] for l in tp.plan_case(tp.lane_case_for(shape, P, st), **st)[0] if l["shard"] == 0]
    assert lanes_of("borrow3") == [(13, 12, 11)]
    assert lanes_of("borrow3", dyn_lanes=2) == [(3, 12, 11), plain]
    assert lanes_of("borrow3", dyn_lanes=1, lane_map=0) == [(3, 4, 11), plain]
    assert lanes_of("borrow3", dyn_lanes=0, lane_map=0) == [plain, plain]
    assert lanes_of("static4") == [(13, 4, 11)]
    assert lanes_of("scatter") == [(10, 13, 8)]
    assert lanes_of("static345") == [plain, plain]
    assert lanes_of("classic") == lanes_of("classic", lane_map=2) == lanes_of("classic+lanes") == [(3, 4, 11)]
    assert lanes_of("classic", lane_map=0) == [plain] and lanes_of("classic", lane_map=11 << 10 | 12 << 5) == [(3, 12, 11)]
    assert lanes_of("classic+lanes", lane_map=11 << 10 | 12 << 5) == [plain]      # a static lane target on bit 4 refuses an explicit code
    assert lanes_of("offtile") == [plain] and lanes_of("offtile", lane_map_min_l=14) == [(3, 4, 11)]
    for P in (1, 2, 4):
        assert lanes_of("borrow3", P) == [(13, 12, 11)] and lanes_of("classic", P) == [(3, 4, 11)]
    for shape in ("borrow3", "static4", "scatter", "classic", "classic+lanes", "offtile"):      # the select on bit 11 is there by default
        assert tp.lane_case_for(shape, 1, {}).name.endswith("sel11=1")
    one, both = (tp.plan_case(tp.final_x_case(b)) for b in (False, True))
    assert one[0][0]["lanes"] == plain and one[0][0]["xframe"] == 1 and one[1] == {"multi": 1}
    assert both[0][0]["lanes"] == (3, 4, 11) and both[0][0]["xframe"] == 1 and both[1] == {"multi": 1, "x": 1}


def test_family_e_x_frame_bits():
    for case in E_CASES:
        (l,), launches, fused = tp.plan_case(case)
        lanes, waves, blocks = l["classes"]
        assert l["lanes"] == (3, 4, 11) and {7, 9} <= set(l["reg"]) and {1, 4, 11} <= set(lanes) and 12 in waves and {13, 14} <= set(blocks)
        assert l["xframe"] == (8 if case.init else 5) and launches.get("x", 0) == (0 if case.init else 3)
        assert fused == l["ops"] + 8


def test_family_f_totals():
    assert sum(4 << k for k in tp.F_SELECTS) == 2556
    (l,), launches, _ = tp.plan_case(tp.budget_case(False))
    assert l["tables"] - 4 == 2556 and l["ops"] == 8 and launches == {"multi": 1}
    case = tp.budget_case(True)
    assert sum((4 if op.kind == "mux" else 1) << len(op.ctrls if op.kind == "mux" else op.qubits) for op in case.ops[:9]) == 2558
    lines, launches, _ = tp.plan_case(case)
    assert [x["ops"] for x in lines] == [8, 2] and [x["mode"] for x in lines] == [2, 1] and launches == {"multi": 2}
    for kind in tp.F_BIG:
        case = tp.big_mux_case(kind)
        lines, launches, _ = tp.plan_case(case)
        assert launches["mux"] >= 1 and all(case.sentinels[0] not in l["members"] for l in lines)
        assert len(case.ops[case.sentinels[0]].ctrls) == 10


def test_family_g_zero_tracking():
    for case in G_CASES:
        (a, b), launches, _ = tp.plan_case(case)
        assert launches == {"multi_init": 1, "multi": 1}
        assert a["init"] == 1 and a["zreg"] != 0 and a["lanes"] == b["lanes"] == (-1, -1, -1)
        assert b["init"] == 0 and b["zreg"] == 3 and b["reg"][:4] == [9, 12, 7, 1] and b["nthreads"] == 128
        assert min(a["reg"]) < 6                               # lane mode off: a target below bit 6 is a register bit


# ---------------------------------------------------------------------------------------------------------------------
# sentinels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", A_CASES + B_CASES + C_CASES + CHAINS + D_CASES[::2] + E_CASES + F_CASES + G_CASES, ids=repr)
def test_dropping_a_sentinel_op_moves_the_state(case):
    assert case.sentinels
    for k in case.sentinels:
        assert case.ops[k].kind in ("mux", "diag")
        assert moved(case, skip=k) > 1e-6, k


@pytest.mark.parametrize("case", [c for c in A_CASES + B_CASES if c.mode == 2], ids=repr)
def test_exchanging_s_or_c_of_one_table_entry_moves_the_state(case):
    """the entry of every sentinel mux that amplitude actually reaches: entry 0 first, else the first that moves anything"""
    for k in case.sentinels:
        for what in ("s", "c"):
            n = case.ops[k].mats.shape[0]
            assert max(moved(case, tp.with_entry_changed(case.ops, k, what, e)) for e in range(min(n, 4))) > 1e-6, (k, what)


@pytest.mark.parametrize("kind", tp.C_PAIRS)
def test_reversing_a_pair_moves_the_state(kind):
    a, b = tp.pair_case(kind, 0), tp.pair_case(kind, 1)
    i, j = a.pair
    for x, y in ((i, j), (j, i)):                              # the same two ops, the same tables, exchanged
        assert (a.ops[x].kind, a.ops[x].target) == (b.ops[y].kind, b.ops[y].target)
        assert np.array_equal(a.ops[x].table if a.ops[x].kind == "diag" else a.ops[x].mats,
                              b.ops[y].table if b.ops[y].kind == "diag" else b.ops[y].mats)
    assert np.array_equal(a.ops[0].mats, b.ops[0].mats) and np.array_equal(a.ops[-1].mats, b.ops[-1].mats)
    assert float(np.abs(final(a) - final(b)).max()) > 1e-6
