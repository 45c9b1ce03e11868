"""Device time of noisy shots with the mid-circuit measurements deferred or taken in place.

    python scripts/time_noisy_measure.py --mode deferred|in_place [--n 10] [--shots 2048] [--runs 2] [--label NAME]

The lowered chain of ``--n`` variables (n - 1 cliques) under the thermal model of time_noisy_kraus.py.
``deferred``: every measurement at the end, n + (n - 1) + 1 qubits per shot (20 for n = 10: ``noisy_sample_hbm``, or
``noisy_sample`` up to 13).  It uses nothing newer than the slot path, so the same script times an older checkout (put it
first on PYTHONPATH).  ``in_place``: what ``run(noisy_measure="in_place")`` hands the engine, n + 2 live qubits.

Every call is bracketed by HIP events on the engine's stream (qsv_timer_begin / _end: uploads, the kernel, the download of
the words); the wall time of the call is reported next to it.  One JSON line per run."""
import argparse
import json
import os
import sys
import time

import numpy as np

if "PYTHONPATH" not in os.environ:
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from qcmrf_amd import QCMRF, _lib, ingest as ing_mod, program, workloads  # noqa: E402
from qcmrf_amd.run_experiment import ibm_like_model                       # noqa: E402
from qcmrf_amd.transpile import transpile                                 # noqa: E402

BASIS = ["cx", "id", "rz", "sx", "x"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("deferred", "in_place"), required=True)
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--shots", type=int, default=2048)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    nm = ibm_like_model("0.001,0.01", 0.02, t1=100.0, t2=80.0, gate_time="35,300")   # T1 100 us, T2 80 us, sx 35 ns, cx 300 ns
    cliques = workloads.chain(args.n)
    theta = workloads.theta_halfnorm(sum(2 ** len(c) for c in cliques))
    T = transpile(QCMRF(cliques, list(theta), with_measurements=True), basis_gates=BASIS)
    t0 = time.perf_counter()
    if args.mode == "deferred":
        ing = ing_mod.ingest(T, noise=nm)
        rec, data = program.encode(ing.ops)
        W, n_measure = ing.num_qubits, 0
        meas = [ing.measure.get(c, -1) for c in range(ing.num_clbits)]
        ro = np.array([ing.readout.get(c, (0.0, 0.0)) for c in range(ing.num_clbits)])
    else:
        from qcmrf_amd.backend import QsvBackend
        ing, rec, data, _, meas, ro, _, _, (_, W, n_measure) = QsvBackend._prepare_noisy(T, nm, "auto", "in_place")
    t_host = time.perf_counter() - t0
    state = "lds" if W <= _lib.NOISY_MAX_QUBITS else "hbm"
    with _lib.Engine(W) as eng:
        fn = eng.noisy_sample if state == "lds" else eng.noisy_sample_hbm
        fn(rec, data, 4, 1, meas, ro)                                    # warm-up: module load, first launch
        for r in range(args.runs):
            t1 = time.perf_counter()
            eng.timer_begin()
            words = fn(rec, data, args.shots, 1984 + r, meas, ro)
            ms = eng.timer_end()
            wall = (time.perf_counter() - t1) * 1e3
            print(json.dumps({"label": args.label, "mode": args.mode, "n": args.n, "circuit_qubits": ing.num_qubits, "W": W,
                              "noisy_state": state, "records": len(rec), "measure_records": n_measure, "kraus_ops": ing.n_kraus,
                              "pauli_ops": ing.n_pauli, "shots": args.shots, "run": r, "ms": round(ms, 3),
                              "wall_ms": round(wall, 3), "us_per_shot": round(ms * 1e3 / args.shots, 2),
                              "distinct_words": int(np.unique(words).size), "host_compile_s": round(t_host, 3)}), flush=True)


if __name__ == "__main__":
    main()
