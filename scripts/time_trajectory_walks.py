"""Both walks of the trajectory mode, alternately, in one job:  python scripts/time_trajectory_walks.py [--cases abc]

Per case one warm-up of each walk (an eighth of the shots), then each walk twice, alternating; the best wall time of the
two is printed with branch_nodes, batches, shots/s and, for the levels walk, the share of the time spent on the leaves
(extraction, last segment, sampling -- all per leaf).  The yardstick is the depth walk of the same build in the same job.
  (a) 6 variables, 60 cliques: W = 67, 8 live qubits, 10 000 shots  -- tiny slots, launch-bound
  (b) chain(14), 2 048 shots
  (c) chain(22): W = 44, 24 live qubits, 4 096 shots                -- 256 MiB slots, 4 per batch, bandwidth-bound
  (d) (e) (f) chain(16), chain(18), chain(20), 4 096 shots: 18, 20 and 22 live qubits, between (b) and (c) -- where the
      two walks cross (not run unless asked for: --cases abcdef)"""
import argparse
import sys
import time

sys.path.insert(0, ".")
from qcmrf_amd import QCMRF, workloads as wl          # noqa: E402
from qcmrf_amd.backend import QsvBackend              # noqa: E402


def cases():
    ring = [[i % 6, (i + 1) % 6] for i in range(60)]
    return {"a": ("W67 ring 6x60", QCMRF(ring, wl.theta_halfnorm(240, scale=0.05)), 10000),
            "b": ("chain(14)", QCMRF(wl.chain(14), wl.theta_halfnorm(wl.dimension(wl.chain(14)), scale=0.25)), 2048),
            "c": ("chain(22)", QCMRF(wl.chain(22), wl.theta_halfnorm(wl.dimension(wl.chain(22)), scale=0.25)), 4096),
            "d": ("chain(16)", QCMRF(wl.chain(16), wl.theta_halfnorm(wl.dimension(wl.chain(16)), scale=0.25)), 4096),
            "e": ("chain(18)", QCMRF(wl.chain(18), wl.theta_halfnorm(wl.dimension(wl.chain(18)), scale=0.25)), 4096),
            "f": ("chain(20)", QCMRF(wl.chain(20), wl.theta_halfnorm(wl.dimension(wl.chain(20)), scale=0.25)), 4096)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="abc")
    ap.add_argument("--seed", type=int, default=1984)
    args = ap.parse_args(argv)
    be = QsvBackend(method="trajectory")
    for key in args.cases:
        name, qc, shots = cases()[key]
        for walk in ("depth", "levels"):
            be.run(qc, shots=max(shots // 8, 1), seed_simulator=args.seed, trajectory_walk=walk).result()
        best = {}
        for rep in range(2):
            for walk in ("depth", "levels"):
                t0 = time.perf_counter()
                res = be.run(qc, shots=shots, seed_simulator=args.seed, trajectory_walk=walk).result()
                dt = time.perf_counter() - t0
                assert sum(res.get_counts().values()) == shots
                best.setdefault(walk, []).append((dt, res.metadata(0)))
        for walk in ("depth", "levels"):
            times = [t for t, _ in best[walk]]
            dt, m = min(best[walk], key=lambda x: x[0])
            extra = "" if walk == "depth" else "  slots %d  max_batch_slots %d  leaf share %.2f" % (
                m["trajectory_slots"], m["max_batch_slots"], m["time_leaves"] / max(m["time_evolve"], 1e-12))
            print("(%s) %-14s %-6s wall %8.3f s (runs %s)  live_qubits %d  segments %d  branch_nodes %d  batches %d  %9.0f shots/s%s"
                  % (key, name, walk, dt, " ".join("%.3f" % t for t in times), m["live_qubits"], m["n_segments"],
                     m["branch_nodes"], m["batches"], shots / dt, extra), flush=True)
        print("(%s) levels / depth: %.2fx faster" % (key, min(t for t, _ in best["depth"]) / min(t for t, _ in best["levels"])), flush=True)
    be.close()


if __name__ == "__main__":
    main()
