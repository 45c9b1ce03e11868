"""Programs for the table-op k_multi passes (MODE 1 / MODE 2: multi_2x2_bit / multi_diag / the INIT scalar shortcut in
qsv_kmulti.h, fed by flush_group in qsv_multi.inc), and a host model of what qsv_exec makes of them.  No GPU import:
tests/test_table_pass_cases.py checks the builders on the CPU, tests/test_gpu_table_pass.py runs them on the device.

``plan_table(ops, L, shard, options)`` walks a program the way qsv_exec does for one shard -- groupable, the X frame,
place_target, group_fits, group_add, flush_group, flush_group_hard -- and returns what the engine must report: one dict per
``[qsv pass]`` trace line (R, mode, init, ops, X-frame bits applied, histogram, rounds, lane map, table entries) and the
launches by kind.  It models programs of init, mux, diag and uncontrolled X; anything that would turn a pass general raises
``NotATablePass`` (those passes belong to _general_pass_cases).  Rules of flush_group a reader of the trace would not guess:

* a table pass runs a gate in EVERY slot of every round (gaps are an identity table), and the histogram counts what is
  uploaded: ``tab_t`` is rounds x R, not the number of muxes; ``tables`` includes the 4 entries of the identity;
* a mux whose target is neither a register bit nor a lane bit rides on a BORROWED lane bit: ``ltab_t`` like a lane target;
* MODE 2 is chosen from the table VALUES (exact zeros in the real off-diagonal and the imaginary diagonal parts), and a
  diagonal anywhere in the pass means MODE 1;
* a pass of one op, with nothing pending, is no pass: it runs as its dedicated kernel (single_shortcut).

MODE 2 tables are [[c0, i s0], [i s1, c1]] with four independent values -- non-unitary on purpose, so that exchanging s0 and
s1, c0 and c1, or the halves of a lane pair is visible -- plus unitary asymmetric entries [[c, i s], [-i s, -c]]."""
import numpy as np

from qcmrf_amd import ir
from _general_pass_cases import Case, rand_state, bit_classes, local_op, r_options, haar, phases   # noqa: F401

TABLE_CPLX = 2560 - 4
DEFAULTS = {"multi_r": 5, "pass_max_ops": 56, "single_shortcut": 1, "lane_targets": 1, "init_prod": 1, "lane_map": 1,
            "lane_map_min_l": 26, "dyn_lanes": 3, "zero_tracking": 0, "xframe": 1, "pass_hints": 1, "implied_zeros": 1}
HIST0 = {"tab_t": 0, "tab_p": 0, "x": 0, "mat": 0, "diag_t": 0, "diag_a": 0, "phase": 0, "ltab_t": 0, "ltab_a": 0, "lx": 0, "lmat": 0}


class NotATablePass(Exception):
    pass


# ---------------------------------------------------------------------------------------------------------------------
# table material
# ---------------------------------------------------------------------------------------------------------------------
def asym(rs):
    """[[c0, i s0], [i s1, c1]]: four values of modulus <= 1, none within 0.2 of 0 or of each other, singular values in
    [0.5, 1.3] (a pass of twenty such tables keeps the state within a few orders of magnitude of 1)"""
    while True:
        v = rs.uniform(-1.0, 1.0, size=4)
        if np.abs(v).min() < 0.2 or min(abs(v[i] - v[j]) for i in range(4) for j in range(i)) < 0.2:
            continue
        c0, s0, s1, c1 = (float(x) for x in v)
        m = np.array([[complex(c0, 0.0), complex(0.0, s0)], [complex(0.0, s1), complex(c1, 0.0)]])
        sv = np.linalg.svd(m, compute_uv=False)
        if sv[-1] >= 0.5 and sv[0] <= 1.3:
            return m


def asym_unitary(rs):
    """[[c, i s], [-i s, -c]], c = cos a, s = sin a, a in [0.3, 0.6]: unitary, c0 != c1 and s0 != s1 by more than 0.2"""
    a = float(rs.uniform(0.3, 0.6)) * float(rs.choice([-1.0, 1.0]))
    c, s = float(np.cos(a)), float(np.sin(a))
    return np.array([[complex(c, 0.0), complex(0.0, s)], [complex(0.0, -s), complex(-c, 0.0)]])


def rx_table(rs, k, unitary_only=False):
    """2^k MODE 2 entries, entry 0 (or a random one for k > 0) unitary asymmetric"""
    mats = [asym_unitary(rs) if unitary_only else asym(rs) for _ in range(2 ** k)]
    mats[int(rs.randint(0, 2 ** k))] = asym_unitary(rs)
    return np.array(mats)


def table(rs, k, mode, unitary_only=False):
    return rx_table(rs, k, unitary_only) if mode == 2 else np.array([haar(rs) for _ in range(2 ** k)])


def is_rx(mats):
    m = np.asarray(mats).reshape(-1, 2, 2)
    return bool((m[:, 0, 0].imag == 0.0).all() and (m[:, 1, 1].imag == 0.0).all() and
                (m[:, 0, 1].real == 0.0).all() and (m[:, 1, 0].real == 0.0).all())


# ---------------------------------------------------------------------------------------------------------------------
# host model
# ---------------------------------------------------------------------------------------------------------------------
class _Group:
    def __init__(self):
        self.ops = []                  # (kind, target, selects, rx-like, table entries, program index)
        self.targets, self.selects, self.lane_targets, self.dyn_targets = [], [], [], []
        self.lane_mode = self.opened = self.init = False
        self.table_cplx = 0
        self.nonmask = 0
        self.xframe = 0


def thread_bits(L, reg, lanepos, zout=0):
    """(lane, wave, block) address bits of a pass: tile_base_thr / tile_base_blk with the pass's inserted bits"""
    ins = set(reg) | set(b for b in range(L) if (zout >> b) & 1) | set(p for p in lanepos if p >= 0)
    free = [b for b in range(L) if b not in ins]
    if lanepos[0] < 0:
        return free[:6], free[6:8], free[8:]
    return free[:3] + list(lanepos), free[3:5], free[5:]


def _lane_map(o, L, g, reg, zin, final):
    """LanePos of the pass (flush_group): borrowed bits first, else the access-pattern map, else the plain map"""
    lp = [-1, -1, -1]
    if g.dyn_targets:
        taken = [False] * 3
        for q in g.lane_targets:
            if q >= 3:
                lp[q - 3], taken[q - 3] = q, True
        d = 0
        for k in (2, 1, 0):
            if d < len(g.dyn_targets) and not taken[k]:
                lp[k], taken[k] = g.dyn_targets[d], True
                d += 1
        for k in range(3):
            if not taken[k]:
                lp[k] = 3 + k
        return lp
    if not (o["lane_map"] and g.lane_mode and zin == 0):
        return lp
    ok = all(q >= 6 for q in reg)
    code = o["lane_map"]
    sr = sorted(reg)
    classic = len(reg) == 5 and sr[0] == 6 and sr[4] == 10
    if code == 1:
        ok = ok and L >= 14 and 5 not in g.lane_targets
        if not classic and L < o["lane_map_min_l"]:
            ok = False
        if final and (g.xframe >> 5) & 1 and not (g.xframe >> 11) & 1:
            ok = False
        code = 11 << 10
    elif code == 2:
        ok = ok and classic and L >= 14 and 5 not in g.lane_targets
        code = 11 << 10
    elif any(q >= 3 for q in g.lane_targets):
        ok = False
    want = []
    for k in range(3):
        if not ok:
            break
        f = (code >> (5 * k)) & 31
        w = f if f else 3 + k
        if w >= 28 or w >= L or w in reg or (f and w < 6) or w in want:
            ok = False
        want.append(w)
    return want if ok else lp


def _rounds(g, reg, lane_index):
    """number of rounds the scheduling loop of flush_group lays the ops out in (a list op joins the round whose gates it
    commutes with; a gate its slot if free and, below a placed higher bit, if it commutes with those gates)"""
    def tmask(i):
        return (1 << g.ops[i][1]) if g.ops[i][1] >= 0 else 0

    def smask(i):
        return tmask(i) | sum(1 << q for q in g.ops[i][2])

    def commute(i, j):
        return not (tmask(i) & smask(j)) and not (tmask(j) & smask(i))
    R = len(reg)
    rounds = [{"gate": [-1] * R, "list": []}]
    bp = 0
    for i, (kind, t, sel, _, _, _) in enumerate(g.ops):
        cur = rounds[-1]
        is_list = kind == "diag" or t not in reg
        if is_list:
            fits = all(gi < 0 or commute(i, gi) for gi in cur["gate"])
        else:
            b = reg.index(t)
            fits = cur["gate"][b] < 0
            if fits and b < bp:
                fits = all(gi < 0 or reg.index(g.ops[gi][1]) <= b or commute(i, gi) for gi in cur["gate"])
        if not fits:
            rounds.append({"gate": [-1] * R, "list": []})
            cur = rounds[-1]
            bp = 0
        if is_list:
            cur["list"].append(i)
        else:
            cur["gate"][reg.index(t)] = i
            bp = max(bp, reg.index(t) + 1)
    return rounds


class _Walk:
    def __init__(self, L, shard, options):
        self.o = dict(DEFAULTS)
        self.o.update(options)
        self.L, self.shard = L, shard
        self.zmask = 0
        self.g = _Group()
        self.passes, self.launch, self.fused = [], {}, 0

    def count(self, kind):
        self.launch[kind] = self.launch.get(kind, 0) + 1

    # -- placement ----------------------------------------------------------------------------------------------------
    def stays_simple(self, op, as_reg):
        kind, t, sel = op[:3]
        if any(q in self.g.targets or q == t for q in sel):
            return False
        return not (as_reg and t >= 0 and t in self.g.selects)

    def high_lanes(self):
        return len(self.g.dyn_targets) + sum(1 for q in self.g.lane_targets if q >= 3)

    def place(self, op):
        g, o, t = self.g, self.o, op[1]
        if t < 0:
            return "none"
        if t in g.targets:
            return "reg_old"
        if g.lane_mode and (t in g.lane_targets or t in g.dyn_targets):
            return "lane_old"
        if g.lane_mode and t < 6:
            if len(g.lane_targets) >= 6 or (t >= 3 and self.high_lanes() >= 3):
                return "reject"
            return "lane_new"
        if len(g.targets) < (o["multi_r"] if self.stays_simple(op, True) else min(o["multi_r"], o.get("general_r", 4))):
            if not self.stays_simple(op, True):
                raise NotATablePass("target %d is a select of the pass" % t)
            return "reg_new"
        if g.lane_mode and t < 28 and self.stays_simple(op, False) and len(g.dyn_targets) < o["dyn_lanes"] and self.high_lanes() < 3:
            return "reject" if any(q < 6 for q in g.targets) else "dyn_new"
        return "reject"

    def fits(self, op, ops_left):
        g = self.g
        pl = self.place(op)                    # (an unopened group has lane_mode = false: every target fits it as a register target)
        if pl == "reject":
            return False
        if not self.stays_simple(op, pl in ("reg_new", "reg_old")):
            raise NotATablePass("a select on a register target")
        if g.table_cplx + op[4] > TABLE_CPLX:
            return False
        cap = min(self.o["pass_max_ops"], 112)
        return len(g.ops) < cap or (ops_left <= cap // 8 and len(g.ops) < 128)

    def add(self, op):
        g = self.g
        if not g.opened:
            g.opened = True
            g.lane_mode = bool(self.o["lane_targets"]) and self.L >= 12 and self.zmask == 0
        pl = self.place(op)
        assert pl != "reject"                  # group_add takes a refused op into the EMPTY group regardless: never for these programs
        if not self.stays_simple(op, pl in ("reg_new", "reg_old")):
            raise NotATablePass("a select on a register target")
        {"lane_new": g.lane_targets, "dyn_new": g.dyn_targets, "reg_new": g.targets}.get(pl, []).append(op[1])
        for q in op[2]:
            if q not in g.selects:
                g.selects.append(q)
        g.table_cplx += op[4]
        g.ops.append(op)

    # -- flush --------------------------------------------------------------------------------------------------------
    def flush(self, final=False):
        g, o, L = self.g, self.o, self.L
        if o["init_prod"] and g.init and g.ops and L >= 14 and not g.xframe and all(op[0] == "diag" for op in g.ops):
            self.count("init_prod")
            self.fused += len(g.ops)
            self.zmask = g.nonmask if final and o["implied_zeros"] else 0
            self.g = _Group()
            return
        if not g.ops:
            if g.init:
                self.zmask = 0
                self.count("init")
            for b in range(L):
                if (g.xframe >> b) & 1:
                    self.count("x")
            self.g = _Group()
            return
        if len(g.ops) == 1 and not g.init and not g.xframe and o["single_shortcut"]:
            self.count(g.ops[0][0])
            self.g = _Group()
            return
        reg = list(g.targets)
        want = min(L, max(len(reg), min(3, o["multi_r"])))
        for ps in range(2):
            for b in range(min(6, L - 1), L):
                if len(reg) < want and b not in reg and (ps == 1 or (b not in g.selects and not (self.zmask >> b) & 1)):
                    reg.append(b)
        if not g.lane_targets:
            for b in range(L):
                if len(reg) < want and b not in reg:
                    reg.append(b)
        if L >= 12:
            want5 = min(5, o["multi_r"])

            def clean(b):
                return 6 <= b < L and b not in reg and b not in g.selects and b not in g.dyn_targets and not (self.zmask >> b) & 1
            while len(reg) < want5 and reg:
                if clean(max(reg) + 1):
                    reg.append(max(reg) + 1)
                elif clean(min(reg) - 1):
                    reg.append(min(reg) - 1)
                else:
                    break
            for b in range(6, L):
                if len(reg) < want5 and clean(b):
                    reg.append(b)
        R = len(reg)
        regmask = sum(1 << q for q in reg)
        zin, zout = self.zmask, self.zmask & ~regmask
        zreg = sum(1 << c for c in range(R) if (zin >> reg[c]) & 1)
        self.zmask = zout
        nzout = bin(zout).count("1")
        lp = _lane_map(o, L, g, reg, zin, final)
        for kind, t, sel, _, _, _ in g.ops:
            if any(q in reg for q in sel):
                raise NotATablePass("a select on a padding register bit")
            if t >= 0 and t not in reg and not (g.lane_mode and (t < 6 or t in lp)):
                raise NotATablePass("target %d has no place" % t)
        rounds = _rounds(g, reg, lp)
        hist = dict(HIST0)
        hist["tab_t"] = len(rounds) * R
        hist["diag_t"] = sum(1 for op in g.ops if op[0] == "diag")
        hist["ltab_t"] = sum(1 for op in g.ops if op[0] == "mux" and op[1] not in reg)
        mode = 2 if all(op[0] == "mux" and op[3] for op in g.ops) else 1
        lanes, waves, blocks = thread_bits(L, reg, lp, zout)
        xsafe = (1 << 62) - 1 if g.init else regmask | sum(1 << b for b in lanes)
        xmask, xleft = g.xframe & xsafe, g.xframe & ~xsafe
        nthreads = (1 << L) >> (R + nzout)
        self.passes.append({"shard": self.shard, "R": R, "mode": mode, "init": int(g.init), "ops": len(g.ops),
                            "xframe": bin(xmask).count("1"), "hist": hist, "rounds": len(rounds), "lanes": tuple(lp),
                            "tables": sum(op[4] for op in g.ops) + 4,
                            # not in the trace: what the case builders and the self-consistency tests look at
                            "reg": reg, "zreg": zreg, "nthreads": nthreads, "xmask": xmask, "final": final,
                            "classes": (lanes, waves, blocks), "members": [op[5] for op in g.ops],
                            "round_lists": [[g.ops[i][5] for i in rd["list"]] for rd in rounds],
                            "sums": bool(final and nthreads % 256 == 0 and nthreads >= 256)})
        self.fused += len(g.ops)
        self.count("multi_init" if g.init else "multi")
        self.g = _Group()
        self.g.xframe = xleft

    def flush_hard(self, final=False):
        self.flush(final)
        if self.g.xframe:
            self.flush()


def plan_table(ops, L, shard=0, options=None):
    """{"passes": [...], "launches": {kind: n}, "fused": n} for one shard"""
    w = _Walk(L, shard, options or {})
    o = w.o
    n = len(ops)
    for i, op in enumerate(ops):
        if op.kind == "init":
            w.flush()
            w.g.xframe = 0
            w.g.init = True
            w.g.nonmask = ~op.mask & ((1 << L) - 1)
            w.zmask = w.g.nonmask if o["zero_tracking"] else 0
            continue
        if getattr(op, "new_pass", False) and o["pass_hints"] and w.g.ops:
            w.flush()
        if op.kind == "x":
            if op.ctrls:
                raise NotATablePass("a controlled X")
            if op.target >= L:
                raise ValueError("X on a shard bit")
            if not (o["xframe"] and not o["zero_tracking"] and w.zmask == 0 and L >= 8):
                raise NotATablePass("an X outside the X frame")
            w.g.xframe ^= 1 << op.target
            w.fused += 1
            continue
        lo = local_op(op, L, shard)
        kind, t, sel = lo
        if kind not in ("mux", "diag"):
            raise NotATablePass(kind)
        cplx = (4 if kind == "mux" else 1) << len(sel)
        rec = (kind, t, sel, kind == "mux" and is_rx(op.mats), cplx, i)
        if o["multi_r"] < 1 or len(sel) > 10 or cplx > TABLE_CPLX:
            w.flush_hard()
            w.count(kind)
            continue
        if not w.fits(rec, n - i):
            w.flush()
        w.add(rec)
    w.flush_hard(True)
    return {"passes": w.passes, "launches": w.launch, "fused": w.fused}


def plan_case(case, **options):
    """the model's answer for every shard of a case: (trace lines in shard order, launches summed, fused gates summed)"""
    o = dict(case.options)
    o.update(options)
    lines, launches, fused = [], {}, 0
    for s in range(case.P):
        p = plan_table(case.ops, case.L, s, o)
        lines += p["passes"]
        fused += p["fused"]
        for k, v in p["launches"].items():
            launches[k] = launches.get(k, 0) + v
    return lines, launches, fused


TRACE_KEYS = ("shard", "R", "mode", "init", "ops", "xframe", "hist", "rounds", "lanes", "tables")


def trace_view(line):
    return dict((k, line[k]) for k in TRACE_KEYS)


def geometry(targets, L, options, lane_targets=(), dyn=(), nonmask=0):
    """bit classes of the pass a program on these targets will be: the model run on one bare mux per target"""
    rs = np.random.RandomState(0)
    ops = ([ir.op_init(((1 << L) - 1) & ~nonmask)] if nonmask else []) + \
          [ir.op_mux([], t, table(rs, 0, 1)) for t in list(targets) + list(dyn) + list(lane_targets) + list(targets)[:1]]
    p = plan_table(ops, L, 0, options)["passes"]
    assert len(p) == 1, p
    return p[0]


def spread(classes, k, avoid=()):
    """k select bits taken in turn from the lane, wave and block bits (whichever exist), none of ``avoid``"""
    pools = [[b for b in c if b not in avoid] for c in classes]
    out, i = [], 0
    while len(out) < k and any(pools):
        pool = pools[i % 3]
        i += 1
        if pool:
            out.append(pool.pop(len(pool) // 2))
    assert len(out) == k, (classes, k)
    return out


def _tcase(name, W, ops, options, P=1, init=False, mode=None, sentinels=(), **extra):
    c = Case(name, W, ops, options, P=P, init=init, sentinels=sentinels)
    c.mode = mode
    for k, v in extra.items():
        setattr(c, k, v)
    return c


# ---------------------------------------------------------------------------------------------------------------------
# A. every instantiation
# ---------------------------------------------------------------------------------------------------------------------
A_TARGETS = {"lane14": [7, 9, 6, 10, 8, 12], "nolane14": [2, 8, 5, 11, 0, 9], "small10": [2, 8, 5, 7, 0, 9]}


def inst_case(R, mode, init, variant, seed=0):
    """One pass k_multi<R, init, mode>: R register targets, each with three muxes (0, 1 and 3 selects over lane, wave and
    block bits, rotated from target to target), in lane mode a mux on each of the six lane bits (one or two selects), and in
    MODE 1 diagonals on 1, 2 and 3 qubits off the register targets, one of them on a lane-target bit.  INIT: the mask leaves
    out every register target at odd R (the scalar shortcut of MODE 2), register target 0 alone at even R (a tile that
    starts with several non-zero amplitudes), and the highest select bit."""
    L = 10 if variant == "small10" else 14
    lane = variant == "lane14"
    rs = np.random.RandomState(100 * R + 10 * mode + int(init) + 1000 * list(A_TARGETS).index(variant) + seed)
    targets = A_TARGETS[variant][:R]
    opts = r_options(min(R, 5), lane_targets=int(lane))       # general_r stops at 5; it plays no part in a table pass
    opts["multi_r"] = R
    geo = geometry(targets, L, opts, lane_targets=range(6) if lane else ())
    assert geo["reg"] == targets
    classes = geo["classes"]
    lane_t = list(range(6)) if lane else []
    ops, marked = [], []
    for ti, t in enumerate(targets):
        for k in ((0, 1, 3), (1, 3, 0), (3, 0, 1))[ti % 3]:
            sel = spread(classes[ti % 3:] + classes[:ti % 3], k, avoid=lane_t[:3])
            ops.append(ir.op_mux(sel, t, table(rs, k, mode)))
        if ti in (0, R - 1):
            marked.append(ops[-1])
    for l in lane_t:
        sel = spread(classes[1:] + classes[:1], 1 + (l & 1), avoid=lane_t)
        ops.append(ir.op_mux(sel, l, table(rs, len(sel), mode)))
        if l in (0, 5):
            marked.append(ops[-1])
    if mode == 1:
        free = [b for b in range(L) if b not in targets]
        ops.insert(2, ir.op_diag([free[-1]], phases(rs, 1)))
        ops.insert(len(ops) // 2, ir.op_diag([free[0], free[-2]], phases(rs, 2)))      # free[0]: a lane-target bit in lane mode
        ops.append(ir.op_diag([free[1], free[len(free) // 2], free[-1]], phases(rs, 3)))
        marked += [ops[2], ops[-1]]
    if init:
        out = targets if R & 1 else targets[:1]
        top = max(q for op in ops if op.kind == "mux" for q in op.ctrls)
        mask = ((1 << L) - 1) & ~sum(1 << q for q in list(out) + [top])
        ops.insert(0, ir.op_init(mask))
    sent = [i for i, op in enumerate(ops) if any(op is m for m in marked)]
    return _tcase("inst R=%d mode=%d init=%d %s" % (R, mode, int(init), variant), L, ops, opts, init=init, mode=mode,
                  sentinels=sent, R=R)


# ---------------------------------------------------------------------------------------------------------------------
# B. INIT branches
# ---------------------------------------------------------------------------------------------------------------------
B_KINDS = ("dead", "one-live", "padding", "round1", "mask0", "full")


def init_case(kind, mode=2, nlane=3, seed=0):
    """init(mask) + one k_multi<5, true, mode> pass at 16 qubits (8 workgroups of 4 waves), register tile 6..10.

    dead      every register bit outside the mask; the round-0 list holds ``nlane`` lane muxes (MODE 2: the scalar shortcut)
    one-live  the same with register bit 8 inside the mask: all_dead is false, the list runs on the tile
    padding   three targets (6, 7, 8), the tile padded with bits 9, 10, which are inside the mask
    round1    a second gate on register bit 6 opens round 1 before the first lane mux: round 0's list is empty
    mask0     init(0): one live amplitude, every other wave and workgroup dead
    full      every qubit in the mask

    Each lane mux has a select on a wave bit and one on a block bit, so the table index differs across the live lanes; lane bit
    2, a wave bit and the top block bit are outside the mask (except for "full"), and lane bit 2 is the target of a lane mux
    from nlane = 3 on: amplitude moves into lanes the init wrote zeros to."""
    L = 16
    rs = np.random.RandomState(40 + 7 * B_KINDS.index(kind) + 100 * mode + nlane + seed)
    targets = [6, 7, 8] if kind == "padding" else [6, 7, 8, 9, 10]
    lane_t = [1, 0, 2, 4, 3, 5][:nlane]
    geo = geometry(targets, L, {}, lane_targets=lane_t)
    assert geo["reg"] == [6, 7, 8, 9, 10]
    lanes, waves, blocks = geo["classes"]
    inside = {"dead": [], "one-live": [8], "padding": [9, 10], "round1": []}.get(kind, [])
    out = [q for q in [6, 7, 8, 9, 10] if q not in inside] + [2, waves[1], blocks[-1]]
    mask = {"mask0": 0, "full": (1 << L) - 1}.get(kind, ((1 << L) - 1) & ~sum(1 << q for q in out))
    ops = [ir.op_init(mask)]
    gates = [ir.op_mux(spread((lanes, waves, blocks), k, avoid=lane_t), t, table(rs, k, mode)) for k, t in zip((1, 0, 3, 1, 2), targets)]
    lane_ops = [ir.op_mux([waves[i % 2], blocks[i % len(blocks)]], l, table(rs, 2, mode)) for i, l in enumerate(lane_t)]
    if kind == "round1":
        ops += gates + [ir.op_mux([blocks[0]], 6, table(rs, 1, mode))] + lane_ops
    else:
        ops += lane_ops[:1] + gates[:2] + lane_ops[1:] + gates[2:]        # lane muxes commute with the gates: all in round 0's list
    sent = [i for i, op in enumerate(ops) if op.kind == "mux" and op.target < 6]
    return _tcase("init %s mode=%d lanes=%d" % (kind, mode, nlane), L, ops, {}, init=True, mode=mode, sentinels=sent,
                  lane_ops=sent, round0=kind != "round1")


# ---------------------------------------------------------------------------------------------------------------------
# C. order-sensitive pairs and long chains
# ---------------------------------------------------------------------------------------------------------------------
C_PAIRS = ("gate-lane", "gate-borrowed", "lane-lane", "diag-lane")


def pair_case(kind, order, seed=0):
    """A pass on the register tile 6..10 (one mux per bit first, so the registers are full) holding one pair that does not
    commute, in the order given (0: a then b; 1: b then a), between a mux before and a mux after it.

    gate-lane      a = mux on register bit 7 with a select on lane bit 2      b = mux on lane bit 2
    gate-borrowed  a = mux on register bit 7 with a select on bit 12         b = mux on bit 12 (a borrowed lane bit)
    lane-lane      a = mux on lane bit 1 with a select on lane bit 4          b = mux on lane bit 4
    diag-lane      a = diagonal on bits 3 and 12                              b = mux on lane bit 3            (MODE 1)"""
    L = 14
    mode = 1 if kind == "diag-lane" else 2
    rs = np.random.RandomState(600 + 10 * C_PAIRS.index(kind) + seed)        # the same tables in both orders
    ops = [ir.op_mux([11], t, table(rs, 1, mode)) for t in (6, 7, 8, 9, 10)]
    if kind == "gate-lane":
        a, b = ir.op_mux([2, 13], 7, table(rs, 2, mode)), ir.op_mux([11], 2, table(rs, 1, mode))
    elif kind == "gate-borrowed":
        a, b = ir.op_mux([12, 0], 7, table(rs, 2, mode)), ir.op_mux([13], 12, table(rs, 1, mode))
    elif kind == "lane-lane":
        a, b = ir.op_mux([4, 11], 1, table(rs, 2, mode)), ir.op_mux([13], 4, table(rs, 1, mode))
    else:
        a, b = ir.op_diag([3, 12], phases(rs, 2)), ir.op_mux([13], 3, table(rs, 1, mode))
    ops += [b, a] if order else [a, b]
    ops.append(ir.op_mux([0], 9, table(rs, 1, mode)))
    return _tcase("pair %s order=%d" % (kind, order), L, ops, {}, mode=mode, sentinels=[5, 6], pair=(5, 6))


def chain_case(N, pass_max_ops=None, seed=0):
    """N MODE 2 muxes on the register tile 6..10 and lane bits 0, 3 with unitary asymmetric tables (a chain of N non-unitary
    ones would leave the scale of the state to chance).  N = 40 with ``same``: one target hit 40 times, 40 rounds."""
    L = 14
    rs = np.random.RandomState(700 + N + seed)
    tg = [6, 7, 8, 9, 10, 0, 3]
    ops = [ir.op_mux([11 + i % 3] if i % 4 else [], tg[i % 7], rx_table(rs, 1 if i % 4 else 0, True)) for i in range(N)]
    opts = {} if pass_max_ops is None else {"pass_max_ops": pass_max_ops}
    return _tcase("chain N=%d cap=%s" % (N, pass_max_ops), L, ops, opts, mode=2, sentinels=[0, N // 2, N - 1])


def same_target_case(seed=0):
    L = 14
    rs = np.random.RandomState(740 + seed)
    ops = [ir.op_mux([11 + i % 3, i % 6], 8, rx_table(rs, 2, True)) for i in range(40)]
    return _tcase("one target 40 times", L, ops, {}, mode=2, sentinels=[0, 17, 39])


# (pass_max_ops, ops, ops per pass): cap = min(pass_max_ops, 112), the last cap / 8 ops of a program ride along up to 128
CHAIN_CUTS = [(200, 112, [112]), (200, 126, [126]), (200, 127, [112, 15]), (None, 63, [63]), (None, 64, [56, 8])]


# ---------------------------------------------------------------------------------------------------------------------
# D. lanes lent, map taken
# ---------------------------------------------------------------------------------------------------------------------
D_SHAPES = {                                   # register targets, the other targets in program order, extras
    "borrow3": ([6, 7, 8, 9, 10], [11, 12, 13, 0, 1, 2]),           # 5 registers + 3 borrowed + 3 static lanes
    "static4": ([6, 7, 8, 9, 10], [11, 4, 13, 2]),                  # a static lane target on bit 4 keeps its lane
    "scatter": ([9, 7, 12, 6, 14], [8, 13, 10]),                    # scattered registers, borrowed bits between them
    "classic": ([6, 7, 8, 9, 10], []),                              # the lane map pattern (lane bit 5 -> bit 11)
    "classic+lanes": ([6, 7, 8, 9, 10], [0, 3, 4]),                 # ... with static lane gates beside it
    "static345": ([6, 7, 8, 9, 10], [3, 4, 5, 11]),                 # lane bits 3, 4, 5 all taken: nothing left to lend
    "offtile": ([7, 8, 9, 10, 12], [1]),                            # not the classic tile: the map from lane_map_min_l on
}
D_SETTINGS = [{}, {"dyn_lanes": 0, "lane_map": 0}, {"dyn_lanes": 1, "lane_map": 0}, {"dyn_lanes": 2}, {"dyn_lanes": 3, "lane_map": 2},
              {"lane_map": 11 << 10 | 12 << 5}, {"lane_map_min_l": 14}, {"dyn_lanes": 1, "lane_map_min_l": 14}]


def lane_case(shape, P=1, mode=2, sel11=True, seed=0):
    """17 qubits: one mux per target with selects on the two top qubits (shard bits from P = 2 on), then a mux on the second
    register target with a select on lane bit 0 and, with ``sel11``, one on the fourth with a select on bit 11 -- lane bit 5's
    place under lane_map = 1, a borrowed bit where bit 11 is a target.  Where a setting makes bit 11 a REGISTER target of a
    later pass (no lane left to lend) that select would turn the pass general: lane_case_for leaves it out there."""
    W = 17
    rs = np.random.RandomState(800 + 10 * list(D_SHAPES).index(shape) + mode + seed)
    regs, others = D_SHAPES[shape]
    ops = [ir.op_mux([W - 1, W - 2], t, table(rs, 2, mode)) for t in regs + others]
    ops.append(ir.op_mux([0], regs[1], table(rs, 1, mode)))
    if sel11:
        ops.append(ir.op_mux([11, W - 1], regs[3], table(rs, 2, mode)))
    n = len(regs + others)
    return _tcase("lanes %s P=%d mode=%d sel11=%d" % (shape, P, mode, int(sel11)), W, ops, {}, P=P, mode=mode,
                  sentinels=[0, n - 1, n] + ([n + 1] if sel11 else []))


def lane_case_for(shape, P, setting, mode=2):
    """the program with the select on bit 11 where every pass stays a table pass under ``setting``, else without it"""
    case = lane_case(shape, P, mode, True)
    try:
        plan_case(case, **setting)
    except NotATablePass:
        case = lane_case(shape, P, mode, False)
    return case


def final_x_case(both, seed=0):
    """the classic tile at 17 qubits with an X pending on bit 5 (both: and on bit 11) when the program ends: with bit 11
    clean the last pass keeps the plain map and stores through the X itself; with both pending the map is taken, bit 11 is
    a lane bit (applied by the pass) and bit 5 a wave bit (left to a swap kernel)"""
    W = 17
    rs = np.random.RandomState(880 + int(both) + seed)
    ops = [ir.op_mux([W - 1, 12], t, table(rs, 2, 2)) for t in (6, 7, 8)]
    ops += [ir.op_x(5)] + ([ir.op_x(11)] if both else [])
    ops += [ir.op_mux([5, 11], t, table(rs, 2, 2)) for t in (9, 10, 6)]
    return _tcase("final X on 5%s" % (" and 11" if both else ""), W, ops, {}, mode=2, sentinels=[0, len(ops) - 1])


# ---------------------------------------------------------------------------------------------------------------------
# E. X frame on table passes
# ---------------------------------------------------------------------------------------------------------------------
def xframe_case(init, mode=2, seed=0):
    """Tile 6..10 at 16 qubits, lane muxes on bits 1 and 4 (the lane map is on: lane bits 0 1 2 3 4 11, wave bits 5 12, block
    bits 13..15).  An uncontrolled X on register bit 7, lane bit 1, wave bit 12 and block bit 14 before the table ops, and on
    register bit 9, lane bit 4, bit 11 (a lane bit under the map) and block bit 13 between them; every later table op has a
    select or its target on one of them.  A read+write pass applies the register and lane bits (5 of 8); the wave and block
    bits stay pending and run as swap kernels after it.  An init pass takes all eight."""
    L = 16
    rs = np.random.RandomState(900 + 2 * mode + int(init) + seed)
    mask = ((1 << L) - 1) & ~((1 << 6) | (1 << 15) | (1 << 2))
    ops = [ir.op_init(mask)] if init else []
    ops += [ir.op_x(q) for q in (7, 1, 12, 14)]
    ops += [ir.op_mux([12, 14], 7, table(rs, 2, mode)), ir.op_mux([1, 13], 6, table(rs, 2, mode)), ir.op_mux([14], 1, table(rs, 1, mode)),
            ir.op_mux([], 8, table(rs, 0, mode))]
    ops += [ir.op_x(q) for q in (9, 4, 11, 13)]
    ops += [ir.op_mux([11, 13], 9, table(rs, 2, mode)), ir.op_mux([12], 4, table(rs, 1, mode)), ir.op_mux([4, 11, 14], 10, table(rs, 3, mode)),
            ir.op_mux([13], 7, table(rs, 1, mode))]
    if mode == 1:
        ops.append(ir.op_diag([1, 11, 14], phases(rs, 3)))
    first = 1 if init else 0
    return _tcase("xframe init=%d mode=%d" % (int(init), mode), L, ops, {}, init=init, mode=mode,
                  sentinels=[first + 4, first + 12, len(ops) - 1])


# ---------------------------------------------------------------------------------------------------------------------
# F. table budget
# ---------------------------------------------------------------------------------------------------------------------
F_SELECTS = (9, 6, 5, 4, 3, 2, 1, 0)
_F_POOL = [0, 1, 2, 3, 4, 5, 11, 12, 13, 14, 15, 16]


def budget_case(extra, seed=0):
    """17 qubits, muxes with 9, 6, 5, 4, 3, 2, 1, 0 selects on targets 6, 7, 8: 2048 + 256 + 128 + 64 + 32 + 16 + 8 + 4 = 2556
    table entries, the most a pass stages.  ``extra``: a one-qubit diagonal (2 entries) and one more mux follow -- they no
    longer fit and form a second pass."""
    W = 17
    rs = np.random.RandomState(1000 + int(extra) + seed)
    ops = [ir.op_mux(_F_POOL[i:i + k] if i + k <= 12 else _F_POOL[:k], (6, 7, 8)[i % 3], rx_table(rs, k)) for i, k in enumerate(F_SELECTS)]
    if extra:
        ops += [ir.op_diag([13], phases(rs, 1)), ir.op_mux([14], 7, rx_table(rs, 1))]
    return _tcase("budget extra=%d" % int(extra), W, ops, {}, mode=2, sentinels=[0, 7] + ([8, 9] if extra else []))


F_BIG = ("alone", "init", "x", "no-shortcut")


def big_mux_case(kind, seed=0):
    """a mux with 10 selects (4096 table entries: more than any pass stages) on target 8, alone, behind an init, behind a
    pending X, and with single_shortcut = 0; a small mux on bit 7 before and after it where the program has no init"""
    W = 17
    rs = np.random.RandomState(1100 + F_BIG.index(kind) + seed)
    big = ir.op_mux([0, 1, 2, 3, 4, 5, 11, 12, 13, 14], 8, rx_table(rs, 10))
    if kind == "alone":
        ops = [big]
    elif kind == "init":
        ops = [ir.op_init(((1 << W) - 1) & ~(1 << 8)), big]
    elif kind == "x":
        ops = [ir.op_x(3), ir.op_x(12), big, ir.op_mux([3], 7, rx_table(rs, 1))]
    else:
        ops = [ir.op_mux([12], 7, rx_table(rs, 1)), big, ir.op_mux([3], 7, rx_table(rs, 1))]
    opts = {"single_shortcut": 0} if kind == "no-shortcut" else {}
    return _tcase("big mux %s" % kind, W, ops, opts, init=kind == "init", mode=2, sentinels=[ops.index(big)])


# ---------------------------------------------------------------------------------------------------------------------
# G. zero tracking
# ---------------------------------------------------------------------------------------------------------------------
def zero_case(mode, seed=0):
    """zero_tracking = 1 at 14 qubits, lane mode off (known-zero qubits).  init on a mask that leaves out bits 2, 7, 9, 12, 13;
    the init pass takes targets 7 (known zero), 6 and 3 (populated); a planner hint opens a second pass on targets 9, 12
    (still known zero: zreg != 0, their halves are not read), 7 and 1 (populated), enumerated over the subspace where bits 2
    and 13 stay zero."""
    L = 14
    rs = np.random.RandomState(1200 + mode + seed)
    out = [2, 7, 9, 12, 13]
    mask = ((1 << L) - 1) & ~sum(1 << q for q in out)
    ops = [ir.op_init(mask),
           ir.op_mux([0, 10], 7, table(rs, 2, mode)), ir.op_mux([11], 6, table(rs, 1, mode)), ir.op_mux([4, 5, 8], 3, table(rs, 3, mode)),
           ir.op_mux([], 7, table(rs, 0, mode)),
           ir.op_mux([0, 11], 9, table(rs, 2, mode)), ir.op_mux([3], 12, table(rs, 1, mode)), ir.op_mux([10, 5], 7, table(rs, 2, mode)),
           ir.op_mux([4], 1, table(rs, 1, mode)), ir.op_mux([8], 9, table(rs, 1, mode))]
    if mode == 1:
        ops.insert(3, ir.op_diag([0, 5], phases(rs, 2)))
        ops.append(ir.op_diag([4, 10, 11], phases(rs, 3)))
    hint = 5 + (mode == 1)
    ops[hint].new_pass = True
    return _tcase("zero tracking mode=%d" % mode, L, ops, {"zero_tracking": 1}, init=True, mode=mode,
                  sentinels=[1, hint, hint + 1, len(ops) - 1], hint=hint)


# ---------------------------------------------------------------------------------------------------------------------
# sentinels: a table with s0 <-> s1 or c0 <-> c1 exchanged in one entry
# ---------------------------------------------------------------------------------------------------------------------
def with_entry_changed(ops, k, what, entry=0):
    """the program with entry ``entry`` of op k's table transposed (``what`` = "s") or with its diagonal exchanged ("c")"""
    op = ops[k]
    mats = np.array(op.mats)
    m = mats[entry].copy()
    mats[entry] = m.T if what == "s" else np.array([[m[1, 1], m[0, 1]], [m[1, 0], m[0, 0]]])
    out = list(ops)
    out[k] = ir.op_mux(op.ctrls, op.target, mats)
    return out
