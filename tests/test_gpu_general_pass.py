"""GPU parity of the general k_multi pass (MODE 0), shape by shape: every program of tests/_general_pass_cases.py is run
as ONE Engine.exec on a seeded random unit state (or from its own init op) and all amplitudes are compared with
oracle.sharded_numpy.NumpyEngine on the same records, 1e-12 * max(1, |want|.max()), the norm within 1e-10.

A case never passes by testing something else: besides the amplitudes it asserts the pass structure, from the engine's
stats (launches of ``multi`` / ``multi_init``, fused_gates) and from the ``[qsv pass]`` line option trace_passes prints
for every pass and shard (R, mode 0, init, ops, X-frame bits and the histogram of the eleven update shapes), against what
the host model of _general_pass_cases.plan expects from the ir ops."""
import re

import numpy as np
import pytest

import _general_pass_cases as gp
from oracle.sharded_numpy import NumpyEngine
from qcmrf_amd import program

pytestmark = pytest.mark.gpu

TRACE = re.compile(r"\[qsv pass\] shard (\d+) R (\d+) mode (\d+) init (\d+) ops (\d+) xframe (\d+) \| tab (\d+)/(\d+) x (\d+) mat (\d+)"
                   r" \| diag (\d+)/(\d+) phase (\d+) \| lane tab (\d+)/(\d+) x (\d+) mat (\d+)")


@pytest.fixture(scope="module")
def lib():
    from qcmrf_amd import _lib
    _lib.load()
    assert _lib.device_count() >= 1
    return _lib


_REF = {}


def reference(case, P=None):
    """(start state or None, amplitudes NumpyEngine leaves, their norm): once per program, shared by its variants"""
    P = case.P if P is None else P
    key = (case.name, P)
    if key not in _REF:
        rec, data = program.encode(case.ops)
        ref = NumpyEngine(case.W, P)
        state = None
        if not case.init:
            state = gp.rand_state(case.W, 11)
            for s in range(P):
                ref.sh[s][:] = state[s << ref.L: (s + 1) << ref.L]
            state.setflags(write=False)
        ref.exec(rec, data)
        want = ref.amplitudes()
        want.setflags(write=False)
        _REF[key] = (state, want, float((np.abs(want) ** 2).sum()))
    return _REF[key]


def run(lib, capfd, case, **options):
    """one exec of the case's program: (stats, trace lines as dicts).  The amplitudes and the norm are checked here."""
    state, want, norm = reference(case, 1 if options.pop("_ref_one_shard", False) else None)
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
        got = eng.amplitudes()
        got_norm = eng.norm()
    lines = []
    for m in TRACE.finditer(err):
        v = [int(x) for x in m.groups()]
        lines.append({"shard": v[0], "R": v[1], "mode": v[2], "init": v[3], "ops": v[4], "xframe": v[5],
                      "hist": dict(zip(gp.SHAPES, v[6:]))})
    dev = float(np.abs(got - want).max())
    tol = 1e-12 * max(1.0, float(np.abs(want).max()))
    print("%s %s: max |got - want| = %.3e (tol %.1e), norm off by %.3e" % (case.name, options, dev, tol, abs(got_norm - norm)))
    assert dev <= tol, (case.name, options, dev)
    assert abs(got_norm - norm) <= 1e-10, (case.name, options, got_norm, norm)
    return st, lines


def launches(st, kind):
    return st["kinds"].get(kind, {"launches": 0})["launches"]


def check_passes(case, st, lines, slices, xframe, init=False):
    """``slices``: the (start, stop) op ranges of the passes, in order; every shard runs each as one pass"""
    want_lines, fused = [], 0
    for s in range(case.P):
        for k, (a, b) in enumerate(slices):
            p = gp.plan(case.ops[a:b], case.L, s, lane_mode=case.lane_mode, xframe=xframe)
            assert p["ops"] >= 2                      # a pass of one op would run as its dedicated kernel
            fused += p["ops"] + p["framed"]
            want_lines.append({"shard": s, "R": case.options["multi_r"], "mode": 0, "init": int(init and k == 0), "ops": p["ops"],
                               "xframe": p["framed"], "hist": p["hist"]})
    key = lambda d: d["shard"]
    assert sorted(lines, key=key) == sorted(want_lines, key=key)
    n_init = case.P if init else 0
    assert launches(st, "multi_init") == n_init
    assert launches(st, "multi") == len(want_lines) - n_init
    return fused


# ---------------------------------------------------------------------------------------------------------------------
# A. shape x register bit x R
# ---------------------------------------------------------------------------------------------------------------------
A_VARIANTS = [("lane", 14, {"xframe": 1, "multi_nt": 0}), ("lane", 14, {"xframe": 0, "multi_nt": 0}),
              ("lane", 14, {"xframe": 1, "multi_nt": 1}), ("lane", 14, {"xframe": 0, "multi_nt": 1}),
              ("nolane", 14, {}), ("nolane", 10, {})]


@pytest.mark.parametrize("variant", A_VARIANTS, ids=lambda v: "%s%d%s" % (v[0], v[1], "".join("-%s%d" % kv for kv in sorted(v[2].items()))))
@pytest.mark.parametrize("R", [1, 2, 3, 4, 5])
def test_every_shape_on_every_register_bit(lib, capfd, R, variant):
    """One pass of k_multi<R, false, 0> in which every register bit 0..R-1 (targets in first-use order) meets tab T, tab P,
    x, mat, phase and both diagonal shapes under every control placement, and every lane bit the four lane shapes
    (_general_pass_cases.shape_case).  Variants: X frame on (uncontrolled X = store-address XOR, no op) and off (a GS_X op
    with an all-ones fire mask), non-temporal form on and off (instantiated for R >= 3), and lane mode off at 14 and at 10
    qubits, where targets below bit 6 are register bits: there the histogram shows the seven register shapes and no lane
    shape.  At R = 1 no second register bit exists, hence no tab P."""
    kind, L, options = variant
    case = gp.shape_case(R, L, kind == "lane")
    st, lines = run(lib, capfd, case, **options)
    fused = check_passes(case, st, lines, [(0, len(case.ops))], xframe=bool(options.get("xframe", 1)))
    assert fused == st["fused_gates"] == len(case.ops)
    for s in gp.SHAPES:
        assert (lines[0]["hist"][s] > 0) == (s in case.must_show), s
    if kind != "lane":
        assert all(lines[0]["hist"][s] == 0 for s in gp.LANE_SHAPES)


# ---------------------------------------------------------------------------------------------------------------------
# B. mask words of the combo table
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combos", [1, 0])
@pytest.mark.parametrize("N,pattern", gp.MASK_CASES)
def test_mask_words_of_the_combo_table(lib, capfd, N, pattern, combos):
    """R = 4 at 16 qubits, 16 workgroups, N masked ops (CCX, controlled phase, masked 2x2) controlled on the top bits so that
    a workgroup class owns word 0 = 0x00000000FFFFFFFF and its sibling the complement ("half": the mask of the memory faults
    of the unfused 34-qubit stream, a sign-extended readfirstlane of a word with bit 31 set), or exactly one bit: 31, 63,
    word 1 bit 0 (op 64), word 1 bit 31 (op 95), op 125 -- the last needs the tail-riding rule of group_fits (126 ops in a
    pass capped at 112).  With general_combos = 0 every workgroup walks the whole list."""
    case = gp.mask_case(N, pattern)
    st, lines = run(lib, capfd, case, general_combos=combos)
    assert check_passes(case, st, lines, [(0, N)], xframe=True) == st["fused_gates"] == N
    assert lines[0]["R"] == 4 and lines[0]["ops"] == N


@pytest.mark.parametrize("combos", [1, 0])
@pytest.mark.parametrize("P", [2, 4])
def test_mask_words_differ_per_virtual_shard(lib, capfd, P, combos):
    """the half pattern with controls on shard bits: a shard's op list, hence its mask words, is its own (32, 64 ops at
    P = 2; 32, 16, 64, 48 at P = 4)"""
    case = gp.mask_case(64, "half", P)
    st, lines = run(lib, capfd, case, general_combos=combos)
    assert check_passes(case, st, lines, [(0, 64)], xframe=True) == st["fused_gates"]
    assert len(set(l["ops"] for l in lines)) >= 2 and max(l["ops"] for l in lines) == 64


@pytest.mark.parametrize("combos", [1, 0])
def test_more_block_bit_controls_than_the_combo_table_holds(lib, capfd, combos):
    """R = 1 at 19 qubits: ten block bits control ops, the table is indexed by the eight most frequent, the kernel's
    exec-mask test alone decides the other two"""
    case = gp.many_block_bits_case()
    assert len(gp.combo_bits(case)[1]) == 2
    st, lines = run(lib, capfd, case, general_combos=combos)
    assert check_passes(case, st, lines, [(0, len(case.ops))], xframe=True) == st["fused_gates"] == len(case.ops)
    assert lines[0]["R"] == 1


# ---------------------------------------------------------------------------------------------------------------------
# C. where a pass is cut
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pass_max_ops,N,passes", gp.CUT_CASES)
def test_where_a_pass_is_cut(lib, capfd, pass_max_ops, N, passes):
    """group_fits: cap = min(pass_max_ops, 112); an op joins a pass of fewer than cap ops, and the last cap / 8 ops of a
    program ride along up to 128.

        pass_max_ops   ops   passes
        default (56)    63   one          (56 + 7 riding)
        default (56)    64   56 + 8
        64              72   one          (64 + 8 riding)
        64              73   64 + 9
        200            126   one          (112 + 14 riding)
        200            127   112 + 15

    The engine's default is 56, not 64: the rows for 64 set the option."""
    case = gp.cut_case(pass_max_ops, N)
    st, lines = run(lib, capfd, case)
    slices = [(sum(passes[:k]), sum(passes[:k + 1])) for k in range(len(passes))]
    assert [l["ops"] for l in lines] == passes
    assert check_passes(case, st, lines, slices, xframe=True) == st["fused_gates"] == N
    assert launches(st, "multi") == len(passes)


# ---------------------------------------------------------------------------------------------------------------------
# D. INIT general passes and fold_init_h
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combos", [1, 0])
@pytest.mark.parametrize("zt", [0, 1])
@pytest.mark.parametrize("L", [14, 16])
def test_init_pass_with_masked_ops(lib, capfd, L, zt, combos):
    """init(mask) then masked ops: one k_multi<R, INIT, 0> pass.  The mask leaves out a register bit, lane bit 3, a wave bit
    and block bits (most waves start dead and skip the list); CX gates carry amplitude onto the lane and the register bit
    that started at zero.  An init pass builds no combo table whatever general_combos says."""
    case = gp.init_masked_case(L, zt)
    st, lines = run(lib, capfd, case, general_combos=combos)
    n = len(case.ops) - 1
    assert check_passes(case, st, lines, [(1, len(case.ops))], xframe=False, init=True) == st["fused_gates"] == n
    assert all(lines[0]["hist"][s] > 0 for s in case.must_show)


@pytest.mark.parametrize("fold", [1, 0])
@pytest.mark.parametrize("zt", [0, 1])
@pytest.mark.parametrize("L", [14, 16])
def test_leading_h_gates_fold_into_the_init_write_or_run_in_the_init_pass(lib, capfd, L, zt, fold):
    """init(0), five H, general ops.  fold_init_h = 1: the H gates join the init write (counted in fused_gates, no op left);
    0: they are the first five ops (mat / lane mat) of the init pass.  Same amplitudes."""
    case = gp.init_h_case(L, zt)
    st, lines = run(lib, capfd, case, fold_init_h=fold)
    k = len(gp.FOLD_QUBITS)
    first = 1 + (k if fold else 0)
    fused = check_passes(case, st, lines, [(first, len(case.ops))], xframe=False, init=True)
    assert lines[0]["ops"] == len(case.ops) - first
    assert st["fused_gates"] == len(case.ops) - 1 == fused + (k if fold else 0)
    if not fold:
        with_h, without = lines[0]["hist"], gp.plan(case.ops[1 + k:], L, lane_mode=case.lane_mode, xframe=False)["hist"]
        assert with_h["mat"] + with_h["lmat"] == without["mat"] + without["lmat"] + k


@pytest.mark.parametrize("fold", [1, 0])
@pytest.mark.parametrize("edge", range(4), ids=["h-on-masked-qubit", "h-after-non-h", "near-h", "controlled-h"])
def test_edges_of_the_h_streak(lib, capfd, edge, fold):
    """What must NOT fold: H on a qubit the mask already holds (H|+> = |0>), an H after the streak was closed by another
    gate, a matrix 1e-13 away from H (applied as given), a controlled H.  Compared with the dense gate-level oracle too."""
    case, folded = gp.streak_cases()[edge]
    st, lines = run(lib, capfd, case, fold_init_h=fold)
    first = 1 + (folded if fold else 0)
    fused = check_passes(case, st, lines, [(first, len(case.ops))], xframe=False, init=True)
    assert st["fused_gates"] == len(case.ops) - 1 == fused + first - 1
    dense = gp.run_dense(case.ops, case.W)
    assert np.abs(reference(case)[1] - dense).max() < 1e-13


@pytest.mark.parametrize("P", [2, 4])
def test_h_on_a_shard_bit_folds_or_is_refused(lib, capfd, P):
    """fold_init_h = 1 makes H on a shard-bit qubit part of every shard's init write.  With 0 the same record is a dense
    gate on a shard bit, which qsv_exec refuses (RuntimeError): the one place where a knob decides whether a program runs
    (noted in include/qsv.h) -- never a silent difference."""
    case = gp.shard_fold_case(P)
    st, lines = run(lib, capfd, case, fold_init_h=1, _ref_one_shard=True)
    fused = check_passes(case, st, lines, [(5, len(case.ops))], xframe=False, init=True)
    assert st["fused_gates"] == fused + 4
    rec, data = program.encode(case.ops)
    with lib.Engine(case.W, devices=(0,) * P) as eng:
        eng.set_option("fold_init_h", 0)
        with pytest.raises(RuntimeError, match="shard bit"):
            eng.exec(rec, data)
