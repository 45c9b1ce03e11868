"""GPU box: what does a post-selected step cost, and what does it deliver?  (run from the root of the tree to measure)

    python scripts/time_post_select.py [--config 4] [--defer -1] [--shots 4096] [--repeats 5] [--steps 20] [--plain-only] [--label NAME]

One step is ``backend.run(qc, shots).result().get_counts()`` on BASELINE config 4 (34 qubits; ``--config 2 --defer 1``:
28 qubits with the state deferred, where one device cannot hold 34).  Per leg: ``--repeats`` windows of ``--steps`` steps
after two warm-up steps, each window's mean, then their median and range.  Legs:

  plain            no post_select (the code every tree has: run this file from a checkout of the parent commit with
                   --plain-only, alternating with this tree, to see that the plain step did not move)
  post_select      every shot from the branch with all clique ancillas 0: step time, time_sample, the path taken,
                   qsv_state_info before and after, and -- one untimed step with trace_passes -- the tiles listed (stderr)
  post_select_list 0   the same with the state realised first: the measured side of the break-even of DESIGN §6

and the usable samples per second of either way of getting Gibbs samples.  The package is imported from the current
directory, so the same file times any checkout."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.getcwd())
from qcmrf_amd import QCMRF, mrf, workloads as wl      # noqa: E402
from qcmrf_amd.backend import QsvBackend               # noqa: E402


def windows(step, repeats, steps):
    for _ in range(2):
        step()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(steps):
            step()                                      # (ends in the host's copy of the words: synchronised)
        out.append((time.perf_counter() - t0) / steps * 1e3)
    return out


def report(name, ms):
    print("%-22s median %.4f ms  range %.4f .. %.4f  windows %s"
          % (name, statistics.median(ms), min(ms), max(ms), " ".join("%.4f" % v for v in ms)), flush=True)
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=4)
    ap.add_argument("--defer", type=int, default=-1, help="engine option defer_state")
    ap.add_argument("--shots", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--label", default="this change", help="what the log calls the checkout being timed")
    args = ap.parse_args()
    name, C = wl.baseline_config(args.config)
    theta = wl.theta_halfnorm(wl.dimension(C))
    qc = QCMRF(C, theta)
    eo = {"defer_state": args.defer}
    be = QsvBackend(engine_options=eo)
    print("# %s, %d qubits, %d shots, defer_state %d, tree: %s" % (name, qc.num_qubits, args.shots, args.defer, args.label), flush=True)
    seed = [0]

    def step(**kw):
        seed[0] += 1
        return be.run(qc, shots=args.shots, seed_simulator=seed[0], **kw).result()

    plain = report("plain", windows(lambda: step().get_counts(), args.repeats, args.steps))
    if args.plain_only:
        be.close()
        return
    post = qc.post_selection()
    psucc = mrf.success_probability(C, theta)
    res = {}
    for leg, opts in (("post_select", eo), ("post_select_list 0", dict(eo, post_select_list=0))):
        ms = windows(lambda: step(post_select=post, engine_options=opts).get_counts(), args.repeats, args.steps)
        res[leg] = report(leg, ms)
        md = step(post_select=post, engine_options=opts).metadata(0)
        ts = [step(post_select=post, engine_options=opts).metadata(0)["time_sample"] * 1e3 for _ in range(args.steps)]
        print("%-22s path %s  probability %.6g (closed form %.6g)  time_sample median %.4f ms  range %.4f .. %.4f"
              % (leg, md["post_select_path"], md["post_select_probability"], psucc, statistics.median(ts), min(ts), max(ts)))
        # qsv_state_info around one conditioned draw on the state a plain step leaves; trace_passes: the engine says on
        # stderr how many tiles it listed
        step(engine_options=dict(opts, trace_passes=1))
        eng, lay = be.last_engine, be.last_plan.layout
        fm = sum(1 << lay[c] for c in post)               # classical bit c <- qubit c in a QCMRF circuit
        before = eng.state_info()
        sys.stderr.flush()
        words, mass = eng.sample_cond(args.shots, 1, None, fm, 0)
        print("%-22s state_info before %s  after %s  mass %.6g" % (leg, before, eng.state_info(), mass), flush=True)
    print("usable samples / s:    post_select %.4g   post_select_list 0 %.4g   plain x success probability %.4g"
          % (args.shots / res["post_select"] * 1e3, args.shots / res["post_select_list 0"] * 1e3,
             args.shots * psucc / plain * 1e3), flush=True)
    be.close()


if __name__ == "__main__":
    main()
