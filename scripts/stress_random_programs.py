"""GPU box: differential stress of qsv_exec's pass construction -- random programs of table ops
(multiplexed 2x2 with RX-like, asymmetric RX-like or general matrices, diagonals), controlled gates, X and phases on
random bits, with and without a leading init, random pass hints and engine options -- against the
numpy engine.  Not part of the test suite (minutes); run after touching qsv_multi.inc.
With sample_shots > 0 every program is also sampled and the words are held to the exact sampling contract
(tests/_sampler_reference.py): the tile layouts drawn here are the walk orders of the tile-order sampler."""
import os
import sys
sys.path.insert(0, ".")
import numpy as np
from qcmrf_amd import _lib, ir, program
from oracle.sharded_numpy import NumpyEngine


def sample_violations(eng, got, shots, seed, exact):
    """draw ``shots`` words from the state ``got`` was read from and return the sampling rules they break: the
    order-free contract over |got|^2, plus "exact" (word equality with the index-order reference, off the shots that lie
    within the tolerance of a prefix boundary) when the sampler walked in index order.  The programs are unnormalised:
    the tolerance scales with the engine's total."""
    tests = os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, "tests")
    if tests not in sys.path:
        sys.path.insert(0, tests)
    import _sampler_reference as sr
    p = got.real * got.real + got.imag * got.imag
    total = eng.norm()
    tol = sr.TOL_REL * total
    r = sr.sorted_uniforms(seed, shots, total)
    x = sr.unshuffle(seed, shots, eng.sample(shots, seed))
    rules = sr.rules_of(sr.check_inverse_cdf(p, r, x, tol, total))
    if exact:
        want, dist = sr.exact_index_order(p, r)
        if ((x != want) & (dist > tol)).any():
            rules.append("exact")
    return rules



def run(n_cases=300, seed=7, verbose=True, only=None, override=None, widths=(14, 15, 16, 17), poison=False, sample_shots=0,
        n_ops=(3, 26)):
    """returns the number of mismatching programs.  n_ops: (low, high) of the number of ops drawn per program, high excluded.  sample_shots: words drawn from every program (seed from the case number)
    and checked shot by shot; a violated rule counts as a mismatch.  widths: state sizes drawn from; at >= 21 qubits the
    workgroups of a pass no longer run all at once (in-place permutations that cross workgroups show)"""
    rs = np.random.RandomState(seed)
    bad = 0
    engines = {}
    for case in range(n_cases):
        W = int(rs.choice(list(widths)))
        P = int(rs.choice([1, 1, 2, 4]))
        key = (W, P)
        if key not in engines:
            engines[key] = _lib.Engine(W, devices=(0,) * P)
        eng = engines[key]
        style = rs.randint(0, 4)          # 0 rx-like simple, 1 general simple, 2 mixed general, 3 init + diagonals
        def mat():
            if style == 0:
                a = rs.rand() * 3
                return np.array([[np.cos(a), -1j * np.sin(a)], [-1j * np.sin(a), np.cos(a)]])
            q, _ = np.linalg.qr(rs.randn(2, 2) + 1j * rs.randn(2, 2))
            return q
        ops = []
        mask = 0
        for q in range(W):
            if rs.rand() < 0.7:
                mask |= 1 << q
        if rs.rand() < 0.7 or style == 3:
            ops.append(ir.op_init(mask))
        for _ in range(int(rs.randint(n_ops[0], n_ops[1]))):
            k = rs.randint(0, 10)
            qs = [int(x) for x in rs.permutation(W)[:4]]
            L = W - (P.bit_length() - 1)
            if qs[0] >= L:                                  # dense targets must be local to a shard
                qs[0] = int(rs.choice([q for q in range(L) if q not in qs[1:]]))
            if style == 3:
                kk = int(rs.randint(1, 5))
                ops.append(ir.op_diag(qs[:kk], np.exp(1j * rs.randn(2 ** kk)) * (0.5 + rs.rand(2 ** kk))))
            elif style in (0, 1) or k < 5:
                nsel = int(rs.randint(0, 4))
                sel = qs[1:1 + nsel]
                if style in (0, 1):
                    # simple passes need selects that are never targets: take them from the top bits
                    sel = [W - 1 - i for i in range(nsel) if W - 1 - i != qs[0]]
                ops.append(ir.op_mux(sel, qs[0], np.array([mat() for _ in range(2 ** len(sel))])) if sel else ir.op_u(qs[0], mat()))
                if style in (0, 1) and qs[0] >= W - 3:
                    ops.pop()
            elif k in (5, 6):
                nc = int(rs.randint(0, 3))
                ops.append(ir.op_x(qs[0], ctrls=qs[1:1 + nc], vals=[int(v) for v in rs.randint(0, 2, size=nc)]))
            elif k == 7:
                kk = int(rs.randint(1, 4))
                ops.append(ir.op_diag(qs[:kk], np.exp(1j * rs.randn(2 ** kk))))
            elif k == 8:
                kk = int(rs.randint(1, 4))
                ops.append(ir.op_mcphase(qs[:kk], float(rs.randn()), vals=[int(v) for v in rs.randint(0, 2, size=kk)]))
            elif rs.rand() < 0.4 and L >= 6:
                # a dense 2..5-qubit gate on local qubits (every form of the matrix-core kernels is among the random options)
                kk = int(rs.randint(2, min(5, L) + 1))
                tq = [int(x) for x in rs.permutation(L)[:kk]]
                u, _ = np.linalg.qr(rs.randn(2 ** kk, 2 ** kk) + 1j * rs.randn(2 ** kk, 2 ** kk))
                ops.append(ir.op_kq(tq, u))
            else:
                nc = int(rs.randint(0, 3))
                ops.append(ir.op_u(qs[0], mat(), ctrls=qs[1:1 + nc], vals=[int(v) for v in rs.randint(0, 2, size=nc)]))
            if ops and rs.rand() < 0.1 and ops[-1].kind != "init":
                ops[-1].new_pass = True
        ops = [o for o in ops if o is not None]
        if not ops or (len(ops) == 1 and ops[0].kind == "init"):
            ops.append(ir.op_diag([0], [1.0, 1.0j]))
        opts = {"multi_r": int(rs.choice([5, 5, 5, 4, 6, 3])), "dyn_lanes": int(rs.choice([3, 3, 0, 1, 2])),
                "lane_map": int(rs.choice([1, 1, 0])), "lane_targets": int(rs.choice([1, 1, 1, 0])),
                "zero_tracking": int(rs.choice([0, 0, 0, 1])), "init_prod": int(rs.choice([1, 1, 0])),
                "pass_hints": int(rs.choice([1, 1, 0])), "fused_sums": int(rs.choice([1, 0])),
                "xframe": int(rs.choice([1, 1, 0])), "multi_nt": int(rs.choice([-1, 1, 0])),
                "init_prod_nt": int(rs.choice([-1, 1])), "pass_budget": int(rs.choice([0, 0, 30, 100])),
                "general_r": int(rs.choice([4, 4, 5, 3, 2, 1])), "general_light_r": int(rs.choice([5, 5, 4, 3])),
                "pass_max_ops": int(rs.choice([64, 64, 8, 200])), "swizzle": int(rs.choice([1, 2, 2, 0])),
                "lane_map_min_l": int(rs.choice([26, 14, 14])),
                "kq_variant": int(rs.choice([-1, -1, 0, 3, 5, 6, 8])), "kq_order": int(rs.choice([1, 1, 0, 2, 4])),
                "kq3_tile": int(rs.choice([1, 1, 0, 2])), "defer_state": int(rs.choice([-1, 1, 1, 0]))}
        # options added later come from a generator of their own, keyed by (seed, case): the programs and the options above
        # of every logged (seed, case) stay what they were
        rs2 = np.random.RandomState([int(seed) & 0xffffffff, case])
        opts.update({"general_combos": int(rs2.choice([1, 1, 0])), "fold_init_h": int(rs2.choice([1, 1, 0])),
                     "lowctl_mask": int(rs2.choice([1, 1, 0])), "single_shortcut": int(rs2.choice([1, 1, 1, 0]))})
        # half of the RX-like programs get ASYMMETRIC RX-like tables [[c, is], [-is, -c]] (unitary, c0 != c1 and s0 != s1: a MODE 2
        # kernel that mixes up the halves of a pair shows), their bare 2x2 gates as muxes without selects so that the pass stays
        # a table pass, and a leading init on a mask of their own where they had none (drawn from rs2, like the options above)
        if style == 0 and rs2.rand() < 0.5:
            def amat():
                a = float(rs2.uniform(0.3, 1.2)) * float(rs2.choice([-1.0, 1.0]))
                return np.array([[complex(np.cos(a), 0.0), complex(0.0, np.sin(a))], [complex(0.0, -np.sin(a)), complex(-np.cos(a), 0.0)]])
            for i, o in enumerate(ops):
                if o.kind in ("mux", "u"):
                    ops[i] = ir.op_mux(o.ctrls, o.target, np.array([amat() for _ in range(2 ** len(o.ctrls))]))
                    ops[i].new_pass = o.new_pass
            if ops[0].kind != "init":
                ops.insert(0, ir.op_init(int(rs2.randint(0, 1 << W))))
        if only is not None and (case != only if only >= 0 else case < -only):
            continue                                       # replay mode (CASE, or -CASE: from that case on): the generator state advances, nothing runs
        if override:
            opts.update(override)
        for kname, v in opts.items():
            eng.set_option(kname, v)
        rec, data = program.encode(ops)
        ref = NumpyEngine(W, P)
        if ops[0].kind != "init":
            ref.init_uniform((1 << W) - 1)
            eng.init_uniform((1 << W) - 1)
        ref.exec(rec, data)
        if poison:
            eng.poison_lds()                              # quiet NaNs in every compute unit's LDS: a read of an unstaged table shows
        eng.exec(rec, data)
        want = ref.amplitudes()
        got = eng.amplitudes()
        err = float(np.abs(got - want).max())
        tol = 1e-12 * max(1.0, float(np.abs(want).max()))
        nrm_ref = float((np.abs(want) ** 2).sum())
        nerr = abs(eng.norm() - nrm_ref)
        if err > tol or nerr > 1e-10 * max(1.0, nrm_ref):
            bad += 1
            print("MISMATCH case %d W=%d P=%d style=%d err=%.3e normerr=%.3e opts=%s" % (case, W, P, style, err, nerr, opts), flush=True)
            print("   ops:", [repr(o) + ("*" if o.new_pass else "") for o in ops], flush=True)
        elif sample_shots > 0:
            rules = sample_violations(eng, got, sample_shots, 1000003 * seed + case, exact=not opts["fused_sums"])
            if rules:
                bad += 1
                print("SAMPLING case %d W=%d P=%d style=%d rules=%s opts=%s" % (case, W, P, style, rules, opts), flush=True)
                print("   ops:", [repr(o) + ("*" if o.new_pass else "") for o in ops], flush=True)
        if verbose and min(widths) >= 24:
            print("case %d W=%d P=%d ok so far (%d mismatches)" % (case, W, P, bad), flush=True)     # slow cases: keep the log alive
        if case % 50 == 49 and verbose:
            print("... %d cases, %d mismatches" % (case + 1, bad), flush=True)
    for e in engines.values():
        e.close()
    return bad


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 300
    only = int(sys.argv[3]) if len(sys.argv) > 3 and sys.argv[3] not in ("big", "poison", "huge") else None
    if len(sys.argv) > 3 and sys.argv[3] == "poison":       # N SEED poison: LDS poisoned before every program
        bad = run(n, int(sys.argv[2]), poison=True)
        print("done: %d cases, %d mismatches" % (n, bad))
        sys.exit(1 if bad else 0)
    if len(sys.argv) > 3 and sys.argv[3] == "huge":         # N SEED huge: 26-27 qubits -- the size-gated forms (non-temporal, swizzle, lane map) with random gates
        bad = run(n, int(sys.argv[2]), widths=(26, 26, 27))
        print("done: %d cases, %d mismatches" % (n, bad))
        sys.exit(1 if bad else 0)
    if len(sys.argv) > 3 and sys.argv[3] == "big":          # N SEED big: wide states
        bad = run(n, int(sys.argv[2]), widths=(21, 22, 23))
        print("done: %d cases, %d mismatches" % (n, bad))
        sys.exit(1 if bad else 0)
    override = dict((kv.split("=")[0], int(kv.split("=")[1])) for kv in sys.argv[4:])      # replay one case: N SEED CASE opt=value ...
    bad = run(n, int(sys.argv[2]) if len(sys.argv) > 2 else 7, only=only, override=override)
    print("done: %d cases, %d mismatches" % (n, bad))
    sys.exit(1 if bad else 0)
