"""Device time of noisy shots per reference graph: the 70 lowered circuits of the reference experiment, 10 000 shots each,
under the depolarizing + readout model (``--model pauli``) or with thermal relaxation added (``--model thermal``).

    python scripts/time_noisy_kraus.py --model pauli|thermal [--shots 10000] [--passes 2] [--label NAME]

Per circuit one ``noisy_sample`` call bracketed by HIP events on the engine's stream (qsv_timer_begin / _end: uploads, the
kernel, the download of the words); host compile (ingest + encode) is timed apart.  One JSON line per pass and graph, and
one per pass in total.  ``--model pauli`` uses nothing newer than the Pauli noise model, so the same script times an older
checkout (put it first on PYTHONPATH)."""
import argparse
import json
import os
import sys
import time

import numpy as np

if "PYTHONPATH" not in os.environ:
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from qcmrf_amd import QCMRF, _lib, ingest as ing_mod, program            # noqa: E402
from qcmrf_amd.run_experiment import ibm_like_model                      # noqa: E402
from qcmrf_amd.transpile import transpile                                # noqa: E402
from qcmrf_amd.workloads import REFERENCE_GRAPHS as GRAPHS               # noqa: E402

BASIS = ["cx", "id", "rz", "sx", "x"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=("pauli", "thermal"), required=True)
    ap.add_argument("--shots", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    if args.model == "pauli":
        nm = ibm_like_model("0.001,0.01", 0.02)
    else:                                                                # T1 100 us, T2 80 us, sx 35 ns, cx 300 ns
        nm = ibm_like_model("0.001,0.01", 0.02, t1=100.0, t2=80.0, gate_time="35,300")
    np.random.seed(1984)
    from scipy.stats import halfnorm
    progs = []
    t0 = time.perf_counter()
    for j, C in enumerate(GRAPHS):
        d = sum(2 ** len(c) for c in C)
        for _ in range(args.reps):
            theta = -halfnorm.rvs(loc=0, scale=0.5, size=d)
            T = transpile(QCMRF(C, theta.tolist(), with_measurements=True), basis_gates=BASIS)
            ing = ing_mod.ingest(T, noise=nm)
            rec, data = program.encode(ing.ops)
            meas = [ing.measure.get(c, -1) for c in range(ing.num_clbits)]
            ro = np.array([ing.readout.get(c, (0.0, 0.0)) for c in range(ing.num_clbits)])
            progs.append((j, ing.num_qubits, rec, data, meas, ro, getattr(ing, "n_kraus", 0), ing.n_pauli))
    t_host = time.perf_counter() - t0
    engines = {}
    for W in sorted({p[1] for p in progs}):
        engines[W] = _lib.Engine(W)
    j, W, rec, data, meas, ro, _, _ = progs[0]
    engines[W].noisy_sample(rec, data, 100, 1, meas, ro)                 # warm-up: module load, first launch
    for ps in range(args.passes):
        ms = {}
        for i, (j, W, rec, data, meas, ro, nk, npauli) in enumerate(progs):
            eng = engines[W]
            eng.timer_begin()
            eng.noisy_sample(rec, data, args.shots, 1984 + i, meas, ro)
            ms.setdefault(j, []).append(eng.timer_end())
        for j in sorted(ms):
            sel = [p for p in progs if p[0] == j]
            print(json.dumps({"label": args.label, "model": args.model, "pass": ps, "graph": j, "W": sel[0][1],
                              "records": int(np.mean([len(p[2]) for p in sel])), "kraus_ops": int(np.mean([p[6] for p in sel])),
                              "pauli_ops": int(np.mean([p[7] for p in sel])), "calls": len(ms[j]),
                              "ms_per_call": round(float(np.mean(ms[j])), 4), "ms_min": round(float(np.min(ms[j])), 4),
                              "ms_max": round(float(np.max(ms[j])), 4)}), flush=True)
        print(json.dumps({"label": args.label, "model": args.model, "pass": ps, "graph": "all", "calls": len(progs),
                          "shots": args.shots, "device_ms_total": round(float(sum(sum(v) for v in ms.values())), 3),
                          "host_compile_s": round(t_host, 3)}), flush=True)
    for e in engines.values():
        e.close()


if __name__ == "__main__":
    main()
