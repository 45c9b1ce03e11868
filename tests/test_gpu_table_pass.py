"""GPU parity of the table-op k_multi passes (MODE 1: any 2x2 tables and diagonals; MODE 2: RX-like tables, half the flops),
shape by shape: every program of tests/_table_pass_cases.py is run as ONE Engine.exec on a seeded random unit state (or from
its own init op) and all amplitudes are compared with oracle.sharded_numpy.NumpyEngine on the same records,
1e-12 * max(1, |want|.max()), the norm within 1e-10 -- the checks of tests/test_gpu_general_pass.py, whose reference cache
this file shares.

A case never passes by testing something else: the ``[qsv pass]`` lines option trace_passes prints (R, mode, init, ops,
X-frame bits, histogram, rounds, lane map, table entries) and the launches by kind must be what the host model
_table_pass_cases.plan_table derives from the ir ops and the options.  With that, the line proves which k_multi<R, INIT, MODE,
NT> ran; every test prints the instantiations it reached."""
import re

import numpy as np
import pytest

import _general_pass_cases as gp
import _table_pass_cases as tp
from qcmrf_amd import program
from test_gpu_general_pass import lib, reference, launches   # noqa: F401  (lib is the fixture)

pytestmark = pytest.mark.gpu

TRACE = re.compile(r"\[qsv pass\] shard (\d+) R (\d+) mode (\d+) init (\d+) ops (\d+) xframe (\d+) \| tab (\d+)/(\d+) x (\d+) mat (\d+)"
                   r" \| diag (\d+)/(\d+) phase (\d+) \| lane tab (\d+)/(\d+) x (\d+) mat (\d+)"
                   r" \| rounds (\d+) lanes (-?\d+)/(-?\d+)/(-?\d+) tables (\d+)")
KINDS = ("multi", "multi_init", "mux", "diag", "x", "init", "init_prod", "1q", "mcphase", "kq")
_REPORT = []


@pytest.fixture(autouse=True)
def _report():
    """what run() has to say -- deviation, trace lines, instantiations reached -- printed once capfd has let go of stdout"""
    del _REPORT[:]
    yield
    if _REPORT:
        print("\n" + "\n".join(_REPORT))


def run(lib, capfd, case, **options):
    """one exec of the case's program, amplitudes and norm checked against the reference, the trace and the launch counts
    against the model: (amplitudes, trace lines, stats)"""
    state, want, norm = reference(case)
    with_sums = options.pop("_tile_sums", False)
    rec, data = program.encode(case.ops)
    opts = dict(case.options)
    opts.update(options)
    with lib.Engine(case.W, devices=(0,) * case.P) as eng:
        for k, v in opts.items():
            eng.set_option(k, v)
        eng.set_option("trace_passes", 1)
        if state is not None:
            eng.set_amplitudes(0, state)
        eng.reset_stats()
        capfd.readouterr()
        eng.exec(rec, data)
        st = eng.stats()
        err = capfd.readouterr().err
        if with_sums:                                           # before anything else reads the state: what the last pass left
            st["tile_sums"] = [eng.tile_sums(s) for s in range(case.P)]
        got = eng.amplitudes()
        got_norm = eng.norm()
    lines = []
    for m in TRACE.finditer(err):
        v = [int(x) for x in m.groups()]
        lines.append({"shard": v[0], "R": v[1], "mode": v[2], "init": v[3], "ops": v[4], "xframe": v[5],
                      "hist": dict(zip(gp.SHAPES, v[6:17])), "rounds": v[17], "lanes": tuple(v[18:21]), "tables": v[21]})
    assert len(lines) == err.count("[qsv pass]"), err
    dev = float(np.abs(got - want).max())
    tol = 1e-12 * max(1.0, float(np.abs(want).max()))
    report = ["%s %s: max |got - want| = %.3e (tol %.1e), norm off by %.3e" % (case.name, options, dev, tol, abs(got_norm - norm))]
    report += ["    " + line.strip() for line in err.splitlines() if "[qsv pass]" in line]
    nt = int(opts.get("multi_nt", -1) > 0)
    report += ["    reached k_multi<%d, %s, %d, %s> : %s" % (l["R"], "true" if l["init"] else "false", l["mode"],
                                                             "true" if nt and l["R"] >= 3 else "false", case.name) for l in lines]
    _REPORT.extend(report)
    assert dev <= tol, (case.name, options, dev)
    assert abs(got_norm - norm) <= 1e-10, (case.name, options, got_norm, norm)
    want_lines, want_launches, fused = tp.plan_case(case, **options)
    key = lambda d: d["shard"]                                  # stable: the passes of a shard stay in order
    assert sorted(lines, key=key) == sorted((tp.trace_view(l) for l in want_lines), key=key)
    assert dict((k, launches(st, k)) for k in KINDS) == dict((k, want_launches.get(k, 0)) for k in KINDS)
    assert st["fused_gates"] == fused
    return got, lines, st


# ---------------------------------------------------------------------------------------------------------------------
# A. every instantiation
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nt", [0, 1])
@pytest.mark.parametrize("init", [False, True], ids=["read", "init"])
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("R", [1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("variant", list(tp.A_TARGETS))
def test_every_instantiation(lib, capfd, variant, R, mode, init, nt):
    """One pass k_multi<R, init, mode, nt> (_table_pass_cases.inst_case): three muxes with 0, 1 and 3 selects on every register
    bit, a mux on every lane bit, diagonals in MODE 1; 14 qubits in lane mode, 14 qubits with lane_targets = 0 and 10 qubits,
    where targets below bit 6 are register bits and R = 5 is a launch of 32 threads.  The non-temporal form exists from R = 3;
    below, multi_nt = 1 must leave the very same amplitudes."""
    case = tp.inst_case(R, mode, init, variant)
    got, lines, st = run(lib, capfd, case, multi_nt=nt)
    assert len(lines) == 1 and (lines[0]["R"], lines[0]["mode"], lines[0]["init"]) == (R, mode, int(init))
    if nt and R < 3:
        plain, _, _ = run(lib, capfd, case, multi_nt=0)
        assert np.array_equal(got, plain)


# ---------------------------------------------------------------------------------------------------------------------
# B. INIT branches
# ---------------------------------------------------------------------------------------------------------------------
B_CASES = ([(k, 2, 3) for k in tp.B_KINDS] + [("dead", 2, n) for n in (1, 2, 4, 5, 6)] + [("one-live", 2, 6), ("dead", 1, 3), ("one-live", 1, 3)])


@pytest.mark.parametrize("kind,mode,nlane", B_CASES, ids=lambda v: str(v))
def test_init_branches(lib, capfd, kind, mode, nlane):
    """init(mask) + one k_multi<5, true, mode> pass (_table_pass_cases.init_case): the scalar shortcut of MODE 2 with 1..6 lane
    muxes in round 0's list, the same with a register bit or the padding bits inside the mask (no shortcut), with the lane muxes
    in round 1 (nothing to shortcut), from init(0) (one live wave in one live workgroup) and from the full mask, and in MODE 1,
    which has no shortcut.  Lane bit 2, a wave bit and a block bit are outside the mask: dead lanes, waves and workgroups."""
    case = tp.init_case(kind, mode, nlane)
    got, lines, st = run(lib, capfd, case)
    assert len(lines) == 1 and lines[0]["init"] == 1 and lines[0]["mode"] == mode and lines[0]["hist"]["ltab_t"] == nlane
    assert lines[0]["rounds"] == (1 if case.round0 else 2)


# ---------------------------------------------------------------------------------------------------------------------
# C. order-sensitive pairs, long chains
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("kind", tp.C_PAIRS)
def test_order_sensitive_pairs(lib, capfd, kind, order):
    """a gate whose select is a lane target / a borrowed-lane target, a lane mux whose select is another lane target, a diagonal
    on a lane target's bit -- each before and after the mux on that bit (test_table_pass_cases.py: the two orders differ)"""
    case = tp.pair_case(kind, order)
    got, lines, st = run(lib, capfd, case)
    assert len(lines) == 1 and lines[0]["ops"] == 8


def test_one_target_forty_times(lib, capfd):
    got, lines, st = run(lib, capfd, tp.same_target_case())
    assert lines[0]["rounds"] == 40


@pytest.mark.parametrize("pass_max_ops,N,passes", tp.CHAIN_CUTS)
def test_long_chains_and_where_they_are_cut(lib, capfd, pass_max_ops, N, passes):
    """table passes at the op cap: 112 ops, 126 (the tail rides along), 127 (112 + 15), and the default cap of 56 (63: one pass,
    64: 56 + 8)"""
    got, lines, st = run(lib, capfd, tp.chain_case(N, pass_max_ops))
    assert [l["ops"] for l in lines] == passes and launches(st, "multi") == len(passes)


# ---------------------------------------------------------------------------------------------------------------------
# D. lanes lent, map taken
# ---------------------------------------------------------------------------------------------------------------------
D_PARAMS = [(s, P, i) for s in tp.D_SHAPES for P in (1, 2, 4) for i in range(len(tp.D_SETTINGS)) if P == 1 or i in (0, 1, 3, 6)]


@pytest.mark.parametrize("shape,P,setting", D_PARAMS, ids=lambda v: str(v))
def test_borrowed_lanes_and_lane_map(lib, capfd, shape, P, setting):
    """17 qubits on 1, 2 and 4 virtual shards, asymmetric tables: dyn_lanes 0..3 against static lane targets on bits 3, 4, 5,
    lane_map 0, 1, 2 and an explicit code, lane_map_min_l at 14 and at its default with a tile that is not bits 6..10, a
    select on bit 11 and on a borrowed bit.  Which bits are lent and whether the map is taken is asserted from the trace's
    ``lanes`` field against the model; test_table_pass_cases.py pins the model's answers."""
    st = tp.D_SETTINGS[setting]
    case = tp.lane_case_for(shape, P, st)
    run(lib, capfd, case, **st)


@pytest.mark.parametrize("both", [False, True], ids=["x5", "x5-x11"])
def test_final_pass_keeps_the_plain_map_for_an_x_on_bit_5(lib, capfd, both):
    case = tp.final_x_case(both)
    got, lines, st = run(lib, capfd, case)
    assert lines[0]["lanes"] == ((3, 4, 11) if both else (-1, -1, -1)) and launches(st, "x") == int(both)


# ---------------------------------------------------------------------------------------------------------------------
# E. X frame
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("init", [False, True], ids=["read", "init"])
def test_x_frame_on_table_passes(lib, capfd, init, mode):
    """an uncontrolled X on a register, a lane, a wave and a block bit before and between asymmetric table ops: a read+write
    pass stores through the register and lane bits (5 of 8; the other three run as swap kernels after it), an init pass
    through all eight"""
    got, lines, st = run(lib, capfd, tp.xframe_case(init, mode))
    assert lines[0]["xframe"] == (8 if init else 5) and launches(st, "x") == (0 if init else 3) and lines[0]["mode"] == mode


# ---------------------------------------------------------------------------------------------------------------------
# F. table budget
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [False, True], ids=["2556", "2558"])
def test_table_budget(lib, capfd, extra):
    """2556 table entries are one pass; a one-qubit diagonal more and the pass is cut"""
    got, lines, st = run(lib, capfd, tp.budget_case(extra))
    assert [l["tables"] for l in lines] == ([2560, 14] if extra else [2560])


@pytest.mark.parametrize("kind", tp.F_BIG)
def test_a_mux_with_ten_selects_never_joins_a_pass(lib, capfd, kind):
    """4096 table entries: its dedicated kernel, whatever is pending"""
    case = tp.big_mux_case(kind)
    got, lines, st = run(lib, capfd, case)
    assert launches(st, "mux") >= 1 and all(l["tables"] <= 2560 for l in lines)
    if kind != "no-shortcut":
        assert launches(st, "multi") == launches(st, "multi_init") == 0


# ---------------------------------------------------------------------------------------------------------------------
# G. zero tracking
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nt", [0, 1])
@pytest.mark.parametrize("mode", [1, 2])
def test_zero_tracking_in_table_passes(lib, capfd, mode, nt):
    """zero_tracking = 1, lane mode off: an init pass, then a pass whose register bits 9 and 12 are still known zero (their
    halves are not read) while bits 7 and 1 are populated"""
    got, lines, st = run(lib, capfd, tp.zero_case(mode), multi_nt=nt)
    assert [l["init"] for l in lines] == [1, 0] and [l["R"] for l in lines] == [3, 5]


# ---------------------------------------------------------------------------------------------------------------------
# H. tile sums a table pass leaves as the program's last pass
# ---------------------------------------------------------------------------------------------------------------------
H_CASES = [("A", 1, False), ("A", 2, False), ("A", 2, True), ("borrow3", 2, 1), ("classic", 2, 2), ("scatter", 2, 1)]


@pytest.mark.parametrize("family,mode,arg", H_CASES, ids=lambda v: str(v))
def test_tile_sums_of_a_final_table_pass(lib, capfd, family, mode, arg):
    """Engine.tile_sums() after a last pass that is a table pass -- R = 5 in lane mode, read and init (arg), and the 17-qubit
    programs with borrowed lanes and the lane map on 1 and 2 virtual shards (arg) -- against math.fsum of |want|^2 of the
    REFERENCE amplitudes over every tile, the tiles being the block bits of the pass as the model gives them, compacted in
    ascending order like the generator's (_tile_sum_model.tile_index).  Tolerance of test_gpu_tile_sums.py, with the number of
    ops in the place of the number of factors; the states are not normalised (non-unitary tables)."""
    import _tile_sum_model as tm
    case = tp.inst_case(5, mode, arg, "lane14") if family == "A" else tp.lane_case_for(family, arg, {}, mode)
    got, lines, st = run(lib, capfd, case, _tile_sums=True)
    want_lines, _, _ = tp.plan_case(case)
    want = reference(case)[1]
    nfac = sum(1 for op in case.ops if op.kind != "init")
    rel = tm.bound(nfac, 5)
    for s in range(case.P):
        last = [l for l in want_lines if l["shard"] == s][-1]
        assert last["sums"] and last["xmask"] == 0
        exact = tm.exact_tile_sums(want[s << case.L:(s + 1) << case.L], last["classes"][2])
        sums = st["tile_sums"][s]
        assert sums.shape == exact.shape == (last["nthreads"] // 256,)
        err = np.abs(sums - exact)
        worst = float((err / np.where(exact > 0, exact, 1.0)).max())
        _REPORT.append("    shard %d: %d tiles, worst relative error of a tile sum %.3g (bound %.3g)" % (s, sums.size, worst, rel))
        assert (err <= rel * exact).all(), (s, worst, rel)
