"""Device time of a dense two-qubit Kraus record: the 70 lowered circuits of the reference experiment, 10 000 shots each,
with an error on ``cx`` only, given in four ways (the legs):

    product    thermal relaxation on both qubits in product form (t.expand(t)): two ``kraus`` records per cx
    dense      the same channel through ``two_qubit_kraus_error``: one ``kraus2`` record per cx (the 3 x 3 = 9 products of its operators)
    coherent   ``--coherent-cx 0.05`` alone: one ``kraus2`` record of m = 1 per cx
    dense+coh  the relaxation with the coherent error composed onto it: still one ``kraus2`` record per cx

    python scripts/time_noisy_kraus2.py [--shots 10000] [--windows 5] [--density-width 10]

Per circuit one ``noisy_sample`` call bracketed by HIP events on the engine's stream (qsv_timer_begin / _end).  A window runs
every leg once, alternating leg by leg inside each circuit, so that drift of the clocks falls on all legs alike; the figure of
a leg and graph is the median over the windows of its mean time per call.  One JSON line per graph, one in total, and one
for ``method="density_matrix"`` (``density_exec`` on the circuits of ``--density-width`` qubits) with and without the
coherent error."""
import argparse
import json
import os
import sys

import numpy as np

if "PYTHONPATH" not in os.environ:
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from qcmrf_amd import QCMRF, _lib, ingest as ing_mod, program            # noqa: E402
from qcmrf_amd.noise import NoiseModel, coherent_unitary_error, thermal_relaxation_error, two_qubit_kraus_error    # noqa: E402
from qcmrf_amd.run_experiment import cx_over_rotation                    # noqa: E402
from qcmrf_amd.transpile import transpile                                # noqa: E402
from qcmrf_amd.workloads import REFERENCE_GRAPHS as GRAPHS               # noqa: E402

BASIS = ["cx", "id", "rz", "sx", "x"]
LEGS = ("product", "dense", "coherent", "dense+coh")


def models(eps):
    t = thermal_relaxation_error(100e3, 80e3, 300.0)                     # T1 100 us, T2 80 us, cx 300 ns
    dense = two_qubit_kraus_error([np.kron(b, a) for a in t.kraus() for b in t.kraus()])
    coh = coherent_unitary_error(cx_over_rotation(eps))
    out = {}
    for leg, e in zip(LEGS, (t.expand(t), dense, coh, dense.compose(coh))):
        nm = NoiseModel()
        nm.add_all_qubit_quantum_error(e, ["cx"])
        out[leg] = nm
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shots", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--coherent-cx", type=float, default=0.05)
    ap.add_argument("--density-width", type=int, default=10)
    args = ap.parse_args()
    nms = models(args.coherent_cx)
    np.random.seed(1984)
    from scipy.stats import halfnorm
    progs = []                                                           # (graph, W, {leg: (rec, data)}, meas, records per leg)
    for j, C in enumerate(GRAPHS):
        d = sum(2 ** len(c) for c in C)
        for _ in range(args.reps):
            theta = -halfnorm.rvs(loc=0, scale=0.5, size=d)
            T = transpile(QCMRF(C, theta.tolist(), with_measurements=True), basis_gates=BASIS)
            enc, meas, W = {}, None, 0
            for leg in LEGS:
                ing = ing_mod.ingest(T, noise=nms[leg])
                enc[leg] = program.encode(ing.ops)
                meas, W = [ing.measure.get(c, -1) for c in range(ing.num_clbits)], ing.num_qubits
            progs.append((j, W, enc, meas))
    engines = {W: _lib.Engine(W) for W in sorted({p[1] for p in progs})}
    j, W, enc, meas = progs[0]
    for leg in LEGS:
        engines[W].noisy_sample(*enc[leg], 100, 1, meas)                 # warm-up: module load, first launch of each kernel
    ms = {leg: {} for leg in LEGS}                                       # leg -> graph -> window -> [ms]
    for w in range(args.windows):
        for i, (j, W, enc, meas) in enumerate(progs):
            eng = engines[W]
            for leg in LEGS:
                eng.timer_begin()
                eng.noisy_sample(*enc[leg], args.shots, 1984 + i, meas)
                ms[leg].setdefault(j, {}).setdefault(w, []).append(eng.timer_end())
    total = {leg: 0.0 for leg in LEGS}
    for j in sorted(ms[LEGS[0]]):
        sel = [p for p in progs if p[0] == j]
        med = {leg: float(np.median([np.mean(v) for v in ms[leg][j].values()])) for leg in LEGS}
        for leg in LEGS:
            total[leg] += med[leg] * len(sel)
        print(json.dumps({"graph": j, "W": sel[0][1], "calls": len(sel), "shots": args.shots,
                          "records": {leg: int(np.mean([len(p[2][leg][0]) for p in sel])) for leg in LEGS},
                          "ms_per_call": {leg: round(med[leg], 4) for leg in LEGS},
                          "dense/product": round(med["dense"] / med["product"], 3),
                          "coherent/product": round(med["coherent"] / med["product"], 3)}), flush=True)
    print(json.dumps({"graph": "all", "calls": len(progs), "shots": args.shots, "windows": args.windows,
                      "device_ms_total": {leg: round(total[leg], 3) for leg in LEGS},
                      "dense/product": round(total["dense"] / total["product"], 3),
                      "coherent/product": round(total["coherent"] / total["product"], 3)}), flush=True)
    for e in engines.values():
        e.close()
    # the density-matrix method on the circuits of one width: the relaxation in product form, with and without the coherent error
    sel = [p for p in progs if p[1] == args.density_width][:args.reps]
    if sel:
        with _lib.Engine(2 * args.density_width) as eng:
            eng.density_exec(*sel[0][2]["product"])
            eng.density_exec(*sel[0][2]["dense+coh"])
            dm = {"product": [], "dense+coh": []}
            for w in range(args.windows):
                for leg in dm:
                    t = []
                    for j, W, enc, meas in sel:
                        eng.timer_begin()
                        eng.density_exec(*enc[leg])
                        t.append(eng.timer_end())
                    dm[leg].append(float(np.mean(t)))
        print(json.dumps({"method": "density_matrix", "W": args.density_width, "circuits": len(sel), "windows": args.windows,
                          "ms_per_circuit": {leg: round(float(np.median(v)), 4) for leg, v in dm.items()}}), flush=True)


if __name__ == "__main__":
    main()
