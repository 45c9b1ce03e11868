"""GPU box: what do all clique marginals of a QCMRF state cost, the old way and the new?  (run from the root of the tree)

    python scripts/time_marginals.py [--configs 1,2,4] [--repeats 5] [--steps 10] [--old-entries 2] [--unconditioned 2]

Per workload (a BASELINE config), in ONE process, the two ways alternately, ``--repeats`` windows each after a warm-up:

  old   the loop over ``QCMRF.expectation_sufficient_statistic`` -- one circuit run, one state write and one full read
        pass per entry -- timed on the first ``--old-entries`` entries of theta and SCALED to all ``dimension`` entries
        (the entries cost the same: every one runs the same circuit and reads the whole state); the log says so
  new   ``QCMRF.marginals``: one run that leaves a deferrable state deferred, one conditioned pass for all cliques

then, for the new way, the parts: ``time_evolve`` of the run, the time of the ``backend.marginals`` call alone, of one
``sample_cond(shots=0)`` mass pass over the same sub-cube, qsv_state_info around the call and -- one untimed call with
trace_passes -- the tiles the engine listed (its own line, on stderr).

``--unconditioned CONFIG``: the pass with nothing fixed (``post_selected=False``: the whole shard is read) on that config's
state with its cliques as groups: device time by qsv_timer_*, achieved bytes/s as 16 * 2^W / time, next to the rates of
``qsv_expect_diag`` (one group's table: the read stream of k_blocksum) and ``qsv_probabilities`` (one group, LDS
atomics) in the same job."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.getcwd())
from qcmrf_amd import QCMRF, mrf, workloads as wl      # noqa: E402
from qcmrf_amd.backend import QsvBackend               # noqa: E402


def windows(step, repeats, steps):
    step()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        out.append((time.perf_counter() - t0) / steps * 1e3)
    return out


def report(name, ms, scale=1.0, note=""):
    ms = [v * scale for v in ms]
    print("%-26s median %.4f ms  range %.4f .. %.4f  windows %s%s"
          % (name, statistics.median(ms), min(ms), max(ms), " ".join("%.4f" % v for v in ms), note), flush=True)
    return statistics.median(ms)


def conditioned(config, args):
    name, C = wl.baseline_config(config)
    theta = wl.theta_halfnorm(wl.dimension(C))
    qc = QCMRF(C, theta)
    be = QsvBackend()
    n, W, dim = qc.num_vertices, qc.num_qubits, qc.dimension
    print("# %s, %d qubits, %d parameters in %d cliques" % (name, W, dim, len(C)), flush=True)
    entries = []
    for Cq in C:
        for y in ((0,) * len(Cq), (1,) * len(Cq)):
            entries.append((Cq, y))
    entries = entries[:args.old_entries]

    def old():
        return [qc.expectation_sufficient_statistic(be, Cq, y)[0] for Cq, y in entries]

    def new():
        return qc.marginals(be)

    t_old, t_new = [], []
    old(), new()
    for _ in range(args.repeats):                       # alternately, window by window
        t_old += windows(old, 1, max(1, args.steps // 5))[0:1]
        t_new += windows(new, 1, args.steps)[0:1]
    a = report("old: loop, all entries", t_old, dim / float(len(entries)),
               "   (timed on %d of %d entries, scaled by %.1f)" % (len(entries), dim, dim / float(len(entries))))
    b = report("new: QCMRF.marginals", t_new)
    mu, ps = new()
    print("%-26s old / new = %.1f   success probability %.6g (closed form %.6g)" % ("", a / b, ps, mrf.success_probability(C, theta)))
    if W <= 28:
        print("%-26s max |mu - exact| = %.3g" % ("", float(np.abs(mu - mrf.marginals(C, theta)).max())))
    # the parts of the new way
    post = qc.post_selection()
    groups = [[n - 1 - v for v in reversed(Cq)] for Cq in C]
    fixed = {q: 0 for q in range(n, W)}
    ev, call, masspass = [], [], []
    for _ in range(args.steps):
        res = be.run(qc, shots=0, post_select=post).result()
        ev.append(res.metadata(0)["time_evolve"] * 1e3)
        eng, lay = be.last_engine, be.last_plan.layout
        fm = sum(1 << lay[q] for q in fixed)
        eng.sync()
        t0 = time.perf_counter()
        be.marginals(groups, fixed)
        call.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        eng.sample_cond(0, 1, None, fm, 0)
        masspass.append((time.perf_counter() - t0) * 1e3)
    for what, v in (("run: time_evolve", ev), ("backend.marginals call", call), ("sample_cond(0) mass pass", masspass)):
        print("%-26s median %.4f ms  range %.4f .. %.4f" % (what, statistics.median(v), min(v), max(v)), flush=True)
    be.run(qc, shots=0, post_select=post, engine_options={"trace_passes": 1})
    eng = be.last_engine
    before = eng.state_info()
    sys.stderr.flush()
    be.marginals(groups, fixed)
    print("%-26s state_info before %s  after %s" % ("backend.marginals", before, eng.state_info()), flush=True)
    be.close()
    return a, b, statistics.median(masspass)


def unconditioned(config, args):
    name, C = wl.baseline_config(config)
    theta = wl.theta_halfnorm(wl.dimension(C))
    qc = QCMRF(C, theta)
    be = QsvBackend()
    n, W = qc.num_vertices, qc.num_qubits
    be.run(qc, shots=0)                                   # the state written
    eng, lay = be.last_engine, be.last_plan.layout
    groups = [[lay[n - 1 - v] for v in reversed(Cq)] for Cq in C]
    nbytes = 16.0 * 2.0 ** W
    print("# unconditioned pass: %s, %d groups, %.1f GiB read" % (name, len(groups), nbytes / 2 ** 30), flush=True)

    def timed(f):
        out = []
        f()
        for _ in range(args.repeats):
            eng.timer_begin()
            f()
            out.append(eng.timer_end())
        return out

    tab = np.zeros(4)
    tab[3] = 1.0
    legs = (("qsv_marginals_cond, %d groups" % len(groups), lambda: eng.marginals_cond(groups)),
            ("qsv_marginals_cond, 1 group", lambda: eng.marginals_cond(groups[:1])),
            ("qsv_expect_diag", lambda: eng.expect_diag(groups[0], tab)),
            ("qsv_probabilities (k=2)", lambda: eng.probabilities(groups[0])))
    for what, f in legs:
        ms = timed(f)
        m = statistics.median(ms)
        print("%-30s device median %.4f ms  range %.4f .. %.4f   %.3f TB/s" % (what, m, min(ms), max(ms), nbytes / m * 1e-9), flush=True)
    be.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="1,2,4")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--old-entries", type=int, default=2)
    ap.add_argument("--unconditioned", type=int, default=2, help="BASELINE config of the unconditioned pass (0: none)")
    args = ap.parse_args()
    for c in [int(x) for x in args.configs.split(",") if x]:
        conditioned(c, args)
    if args.unconditioned:
        unconditioned(args.unconditioned, args)


if __name__ == "__main__":
    main()
