"""GPU box: the sampling half of a 34-qubit step, part by part, with host timers (run from the repo root).

200 calls each, the program run and the device drained before every timed call (so every draw starts from a fresh state, as
in a step): ``sample`` (qsv_sample), ``sample_unordered`` (qsv_sample_unordered), and the native counts function on the
words drawn.  Then, on those words, ``np.unique``, ``_format_keys`` and the native function with one register and with
registers of 14 + 20 bits, and what the dict alone costs (``dict(zip(keys, counts))`` over ready-made keys).
--config N: BASELINE config N instead of the default 34-qubit workload."""
import argparse
import sys
import time

sys.path.insert(0, ".")
import numpy as np

from qcmrf_amd import QCMRF, program, workloads as wl
from qcmrf_amd import backend as bk

ap = argparse.ArgumentParser()
ap.add_argument("--config", type=int, default=4)
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--shots", type=int, default=4096)
args = ap.parse_args()

name, C = wl.baseline_config(args.config)
qc = QCMRF(C, wl.theta_halfnorm(wl.dimension(C)))
be = bk.QsvBackend()
res = be.run(qc, shots=args.shots, seed_simulator=1).result()
eng, pl = be.last_engine, be.last_plan
ing, _ = be.compile(qc)
rec, data = program.encode(pl.ops)
W = qc.num_qubits
clist = sorted(ing.measure)
meas = [-1] * (clist[-1] + 1)
for c in clist:
    meas[c] = pl.layout[ing.measure[c]]
print("%s: %d qubits, %d shots, counts_path %s, deferred %s" % (name, W, args.shots, res.metadata(0)["counts_path"], eng.state_info()["deferred"]))


def stat(ts):
    ts = np.asarray(ts) * 1e3
    return "median %.3f  min %.3f  max %.3f ms" % (np.median(ts), ts.min(), ts.max())


def fresh(f, n=args.calls):
    """f() timed n times, each after the program has run again and the device is idle"""
    ts = []
    for i in range(n + 5):
        eng.exec(rec, data)
        eng.sync()
        t0 = time.perf_counter()
        r = f(i)
        ts.append(time.perf_counter() - t0)
    return ts[5:], r


def host(f, n=args.calls):
    ts = []
    for _ in range(n + 5):
        t0 = time.perf_counter()
        r = f()
        ts.append(time.perf_counter() - t0)
    return ts[5:], r


ts, words = fresh(lambda i: eng.sample(args.shots, 100 + i, meas))
print("sample                      %s" % stat(ts))
ts, unordered = fresh(lambda i: eng.sample_unordered(args.shots, 100 + i, meas))
print("sample_unordered            %s" % stat(ts))
assert np.array_equal(np.sort(words), np.sort(unordered))
ts, _ = fresh(lambda i: bk._counts_of(eng.sample_unordered(args.shots, 100 + i, meas), None, ing.num_clbits, ing.creg_sizes))
print("sample_unordered + counts   %s" % stat(ts))
bk.use_native_counts(False)
ts, _ = fresh(lambda i: bk._counts_of(eng.sample(args.shots, 100 + i, meas), None, ing.num_clbits, ing.creg_sizes))
print("sample + Python counts      %s   (the parent's sampling half)" % stat(ts))
bk.use_native_counts(True)

two = [("a", 14), ("b", W - 14)]
for label, cregs in (("one register", ing.creg_sizes), ("registers 14 + %d" % (W - 14), two)):
    print("on the %d words drawn, %s:" % (words.size, label))
    ts, (uv, uc) = host(lambda: np.unique(words, return_counts=True))
    print("  np.unique                 %s (%d keys)" % (stat(ts), uv.size))
    ts, ref = host(lambda: bk._format_keys(uv, uc, W, cregs))
    print("  _format_keys              %s" % stat(ts))
    ts, got = host(lambda: bk._counts_native.counts_dict(words, None, W, cregs))
    print("  native counts_dict        %s" % stat(ts))
    assert list(got.items()) == list(ref.items())
    keys, vals = list(ref.keys()), list(ref.values())
    ts, _ = host(lambda: dict(zip(keys, vals)))
    print("  dict(zip(keys, counts))   %s" % stat(ts))
be.close()
