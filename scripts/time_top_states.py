"""GPU box: what do the most probable configurations of a QCMRF state cost?  (run from the root of the tree)

    python scripts/time_top_states.py [--configs 1,2,4] [--repeats 5] [--steps 10] [--unconditioned 2] > profiles/top_states.log

Per workload (a BASELINE config), in ONE process, three calls alternately, ``--repeats`` windows each after a warm-up:

  map k=1    ``QCMRF.map_states(k=1)``: one run that leaves a deferrable state deferred, one conditioned selection pass
             (qsv_top_cond) and one mass pass (qsv_marginals_cond without groups) over the same sub-cube
  map k=64   the same with the 64 most probable configurations
  marginals  ``QCMRF.marginals`` on the same circuit: the same run and one conditioned pass for all cliques

then the parts of ``map_states``: ``time_evolve`` of the run, the ``backend.top_states`` call alone for k = 1 and 64, the
mass pass alone, and qsv_state_info around the call.  Up to 28 qubits the result is compared with ``mrf.map_states``.

``--unconditioned CONFIG``: the pass with nothing fixed on that config's stored state, device time by qsv_timer_*
around the whole call, alternately call by call, bytes/s as 16 * 2^W / time.  First on the state as the run leaves it --
the half the generator knows to be zero is not stored (``implied_zeros``) and neither ``qsv_top_cond`` (k = 1, 8, 64) nor
the one-group ``qsv_marginals_cond`` loads it; then, after ``qsv_expect_diag`` has had the zeros written, the same calls
and ``qsv_expect_diag`` on the fully stored state."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.getcwd())
from qcmrf_amd import QCMRF, mrf, workloads as wl      # noqa: E402
from qcmrf_amd.backend import QsvBackend               # noqa: E402


def window(step, steps):
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    return (time.perf_counter() - t0) / steps * 1e3


def report(name, ms, note=""):
    print("%-26s median %.4f ms  range %.4f .. %.4f  windows %s%s"
          % (name, statistics.median(ms), min(ms), max(ms), " ".join("%.4f" % v for v in ms), note), flush=True)
    return statistics.median(ms)


def conditioned(config, args):
    name, C = wl.baseline_config(config)
    theta = wl.theta_halfnorm(wl.dimension(C))
    qc = QCMRF(C, theta)
    be = QsvBackend()
    n, W = qc.num_vertices, qc.num_qubits
    print("# %s, %d qubits, %d variables, %d cliques" % (name, W, n, len(C)), flush=True)
    legs = (("map k=1: QCMRF.map_states", lambda: qc.map_states(be, k=1)),
            ("map k=64: QCMRF.map_states", lambda: qc.map_states(be, k=64)),
            ("QCMRF.marginals", lambda: qc.marginals(be)))
    times = [[] for _ in legs]
    for _, f in legs:
        f()
    for _ in range(args.repeats):                       # alternately, window by window
        for t, (_, f) in zip(times, legs):
            t.append(window(f, args.steps))
    med = [report(what, t) for t, (what, _) in zip(times, legs)]
    x, p, pc = qc.map_states(be, k=64)
    print("%-26s MAP state %s  p %.6g  p_condition %.6g (closed form %.6g)"
          % ("", "".join(map(str, x[0])), p[0], pc, mrf.success_probability(C, theta)))
    if W <= 28:
        wx, wp = mrf.map_states(C, theta, k=64)
        print("%-26s equal to mrf.map_states: %s, max |p - exact| = %.3g" % ("", bool(np.array_equal(x, wx)), float(np.abs(p - wp).max())))
    # the parts
    post = qc.post_selection()
    fixed = {q: 0 for q in range(n, W)}
    ev, top1, top64, masspass = [], [], [], []
    for _ in range(args.steps):
        res = be.run(qc, shots=0, post_select=post).result()
        ev.append(res.metadata(0)["time_evolve"] * 1e3)
        be.last_engine.sync()
        for k, out in ((1, top1), (64, top64)):
            t0 = time.perf_counter()
            be.top_states(k, fixed)
            out.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        be.marginals([[]], fixed)
        masspass.append((time.perf_counter() - t0) * 1e3)
    for what, v in (("run: time_evolve", ev), ("backend.top_states k=1", top1), ("backend.top_states k=64", top64),
                    ("mass pass (marginals [[]])", masspass)):
        print("%-26s median %.4f ms  range %.4f .. %.4f" % (what, statistics.median(v), min(v), max(v)), flush=True)
    be.run(qc, shots=0, post_select=post)
    eng = be.last_engine
    before = eng.state_info()
    be.top_states(64, fixed)
    print("%-26s state_info before %s  after %s" % ("backend.top_states", before, eng.state_info()), flush=True)
    be.close()
    return med


def unconditioned(config, args):
    name, C = wl.baseline_config(config)
    theta = wl.theta_halfnorm(wl.dimension(C))
    qc = QCMRF(C, theta)
    be = QsvBackend()
    n, W = qc.num_vertices, qc.num_qubits
    be.run(qc, shots=0)                                   # the state written
    eng, lay = be.last_engine, be.last_plan.layout
    group = [lay[n - 1 - v] for v in reversed(C[0])]
    nbytes = 16.0 * 2.0 ** W
    print("# unconditioned pass: %s, stored, %.1f GiB, group %s" % (name, nbytes / 2 ** 30, group), flush=True)
    tab = np.zeros(4)
    tab[3] = 1.0
    readers = (("qsv_marginals_cond, 1 group", lambda: eng.marginals_cond([group])),
               ("qsv_top_cond, k = 1", lambda: eng.top_cond(1)),
               ("qsv_top_cond, k = 8", lambda: eng.top_cond(8)),
               ("qsv_top_cond, k = 64", lambda: eng.top_cond(64)))

    def series(legs):
        for _, f in legs:
            f()
        times = [[] for _ in legs]
        for _ in range(args.repeats):                     # alternately, call by call
            for t, (_, f) in zip(times, legs):
                eng.timer_begin()
                f()
                t.append(eng.timer_end())
        for t, (what, _) in zip(times, legs):
            m = statistics.median(t)
            print("%-30s device median %.4f ms  range %.4f .. %.4f   %.3f TB/s (16 B x 2^%d / time)"
                  % (what, m, min(t), max(t), nbytes / m * 1e-9, W), flush=True)

    print("## the state as the run leaves it: the half the generator knows to be zero is not stored (implied_zeros, the default)"
          " and these readers do not load it", flush=True)
    series(readers)
    print("## after qsv_expect_diag, which has the implied zeros written: every amplitude stored, every amplitude loaded", flush=True)
    series((("qsv_expect_diag", lambda: eng.expect_diag(group, tab)),) + readers)
    be.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="1,2,4")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--unconditioned", type=int, default=2, help="BASELINE config of the unconditioned pass (0: none)")
    args = ap.parse_args()
    for c in [int(x) for x in args.configs.split(",") if x]:
        conditioned(c, args)
    if args.unconditioned:
        unconditioned(args.unconditioned, args)


if __name__ == "__main__":
    main()
