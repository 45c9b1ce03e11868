"""GPU box: what do the conditional clique marginals of B evidence rows cost, row by row and in one batched call?
(run from the root of the tree)

    python scripts/time_marginals_rows.py [--configs 1,2,4] [--rows 256,4096] [--repeats 5] [--hidden 0.3]

Per workload (a BASELINE config, as scripts/time_marginals.py) the Gibbs state is prepared ONCE (``run(shots=0,
post_select=...)``: at 34 qubits the state stays deferred), then, in one process and on that state, alternately,
``--repeats`` windows each after a warm-up:

  loop     one ``backend.marginals(groups, fixed)`` call per row, B + 1 calls: the only way there was
  batched  ONE ``backend.marginals_rows(groups, fixed_rows)`` call over the same B + 1 conditions

The rows are B Gibbs samples (``mrf.gibbs_pmf``, seeded), every entry hidden with probability ``--hidden``; every row
fixes the ancillas and the AND scratch qubit to 0, the extra row fixes those alone.  Both entry points take at most 28
fixed bits local to a shard: at 34 qubits (20 ancilla bits) a row may observe 8 variables, and a sampled row that observes
more has the surplus hidden as well (seeded; the log counts those rows).  Reported: the windows, the medians,
the time per row of both, and the requirement of rank -- every window of the batched call below every window of the
loop -- as PASS or FAIL.  Then the device timeline, by qsv_timer_begin/end: the sum over the rows of the single calls'
spans (events on the stream around each call: copies, kernels and the gaps the host leaves between them) against the
span of the batched call; and the kernels alone, by the engine's profiling events around every launch group (the chunk
kernel and its folds; the tile listing of a deferred state is not part of it).  What the first comparison saves beyond
the last is launch, copy and wait latency.
The two results are compared byte for byte on the way."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.getcwd())
from qcmrf_amd import QCMRF, mrf, workloads as wl      # noqa: E402
from qcmrf_amd.backend import QsvBackend               # noqa: E402


def sample_rows(C, theta, B, hidden, seed, max_observed):
    """(rows, number of rows trimmed): a row that observes more than ``max_observed`` variables has the surplus hidden too
    (seeded): the entry points take at most 28 fixed bits local to a shard, the ancillas included"""
    n = mrf.num_vertices(C)
    p, _ = mrf.gibbs_pmf(C, theta)
    rs = np.random.RandomState(seed)
    xid = rs.choice(p.size, size=B, p=p / p.sum())
    rows = np.array([[(x >> (n - 1 - v)) & 1 for v in range(n)] for x in xid], dtype=np.int64)
    rows[rs.random_sample(rows.shape) < hidden] = -1
    trimmed = 0
    for row in rows:
        seen = np.flatnonzero(row >= 0)
        if seen.size > max_observed:
            row[rs.choice(seen, size=seen.size - max_observed, replace=False)] = -1
            trimmed += 1
    return rows, trimmed


def line(name, ms, B):
    print("%-22s median %10.4f ms  range %10.4f .. %10.4f  per row %8.3f us  windows %s"
          % (name, statistics.median(ms), min(ms), max(ms), statistics.median(ms) / B * 1e3, " ".join("%.4f" % v for v in ms)), flush=True)


def workload(config, args):
    name, C = wl.baseline_config(config)
    theta = wl.theta_halfnorm(wl.dimension(C))
    qc = QCMRF(C, theta)
    n, W = qc.num_vertices, qc.num_qubits
    be = QsvBackend()
    be.run(qc, shots=0, post_select=qc.post_selection())
    eng = be.last_engine
    print("# %s, %d qubits, %d cliques; state_info after the run %s" % (name, W, len(C), eng.state_info()), flush=True)
    groups = [[n - 1 - v for v in reversed(Cq)] for Cq in C]
    anc = {q: 0 for q in range(n, W)}
    verdicts = []
    for B in args.rows:
        rows, trimmed = sample_rows(C, theta, B, args.hidden, 1984 + B, 28 - len(anc))
        fixed_rows = [{**anc, **{n - 1 - v: int(r[v]) for v in range(n) if r[v] >= 0}} for r in rows] + [anc]
        nrows = len(fixed_rows)

        def loop():
            return [be.marginals(groups, f) for f in fixed_rows]

        def batched():
            return be.marginals_rows(groups, fixed_rows)

        one, (out, mass) = loop(), batched()                                  # warm-up, and the contract on the way
        same = all(np.concatenate(p).tobytes() == out[r].tobytes() and m == mass[r] for r, (p, m) in enumerate(one))
        before = eng.state_info()
        t_loop, t_batch = [], []
        for _ in range(args.repeats):                                          # alternately, window by window
            eng.sync()
            t0 = time.perf_counter()
            loop()
            t_loop.append((time.perf_counter() - t0) * 1e3)
            eng.sync()
            t0 = time.perf_counter()
            batched()
            t_batch.append((time.perf_counter() - t0) * 1e3)
        after = eng.state_info()
        print("## B = %d (+1 row for the denominator), %.1f variables observed per row on average, %d rows trimmed to %d observed "
              "(28 fixed bits at most, %d of them ancillas): rows equal the single calls byte for byte: %s"
              % (B, float((rows >= 0).sum(axis=1).mean()), trimmed, 28 - len(anc), len(anc), same))
        line("loop of marginals", t_loop, nrows)
        line("one marginals_rows", t_batch, nrows)
        ok = max(t_batch) < min(t_loop)
        verdicts.append(ok and same)
        print("%-22s loop / batched = %.1f (medians); every batched window below every loop window: %s"
              % ("", statistics.median(t_loop) / statistics.median(t_batch), "PASS" if ok else "FAIL"))
        print("%-22s state_info before the windows %s  after %s" % ("", before, after), flush=True)
        # the device time alone
        d_loop, d_batch = [], []
        for _ in range(args.repeats):
            tot = 0.0
            for f in fixed_rows:
                eng.timer_begin()
                be.marginals(groups, f)
                tot += eng.timer_end()
            d_loop.append(tot)
            eng.timer_begin()
            batched()
            d_batch.append(eng.timer_end())
        line("device: sum of singles", d_loop, nrows)
        line("device: batched", d_batch, nrows)
        # the kernels alone: HIP events around every launch group (the chunk kernel and its folds), summed by the engine
        k_loop, k_batch = [], []
        eng.set_profiling(True)
        for _ in range(args.repeats):
            eng.reset_stats()
            loop()
            k_loop.append(eng.stats()["kinds"]["prob"]["ms"])
            eng.reset_stats()
            batched()
            k_batch.append(eng.stats()["kinds"]["prob"]["ms"])
        eng.set_profiling(False)
        line("kernels: singles", k_loop, nrows)
        line("kernels: batched", k_batch, nrows)
    be.close()
    return verdicts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="1,2,4")
    ap.add_argument("--rows", default="256,4096")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--hidden", type=float, default=0.3)
    args = ap.parse_args()
    args.rows = [int(x) for x in args.rows.split(",") if x]
    verdicts = []
    for c in [int(x) for x in args.configs.split(",") if x]:
        verdicts += workload(c, args)
    print("# rank requirement (every window of the batched call below every window of the loop, equal bytes) at every "
          "width and B: %s" % ("PASS" if all(verdicts) else "FAIL"))


if __name__ == "__main__":
    main()
