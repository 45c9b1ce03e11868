"""Device time of noisy shots whose trajectories live in device memory (``noisy_sample_hbm``).

    python scripts/time_noisy_hbm.py [--part a|b|ab] [--shots 10000] [--reps 2] [--records 400] [--runs 1] [--label NAME]

(a) W <= 13: the lowered reference graphs under the depolarizing + readout model (the programs of time_noisy_kraus.py
    --model pauli), ``--shots`` shots each, through ``noisy_sample`` and ``noisy_sample_hbm`` alternately.  The LDS path is
    the yardstick: the ratio is what the slot costs.
(b) W = 14, 16, 18, 20: the first ``--records`` records of the lowered chain of W / 2 variables under the same model (the
    whole chain is 3400 to 5100 records: minutes of device time at W = 20), with the grid at its default and at 1.
    Per op a trajectory streams 32 x 2^W bytes (read + write); the figure is set against that volume at 8 TB/s.  An identity
    Pauli draw costs nothing, so "ops" counts the records that touch the state: all but the Pauli records, plus the
    expected number of non-identity draws.

Every call is bracketed by HIP events on the engine's stream (qsv_timer_begin / _end: uploads, the kernel, the download of
the words); the wall time of the call, which adds the allocation of the slots, is reported next to it.  One JSON line per
measurement."""
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
HBM_BYTES_PER_S = 8e12
CHAIN_SHOTS = {14: (4096, 16), 16: (2048, 8), 18: (2048, 4), 20: (2048, 2)}     # W -> shots at (default grid, grid 1)


def lowered(cliques, theta, nm):
    T = transpile(QCMRF(cliques, list(theta), with_measurements=True), basis_gates=BASIS)
    ing = ing_mod.ingest(T, noise=nm)
    rec, data = program.encode(ing.ops)
    meas = [ing.measure.get(c, -1) for c in range(ing.num_clbits)]
    ro = np.array([ing.readout.get(c, (0.0, 0.0)) for c in range(ing.num_clbits)])
    return ing.num_qubits, rec, data, meas, ro


def state_ops(rec, data):
    """records that stream the state once per shot: every non-Pauli record, and each Pauli record with the probability
    that its draw is not the identity"""
    pauli = rec["kind"] == _lib.OP_PAULI
    p_id = np.array([data[int(o)] for o in rec["data_off"][pauli]])
    return float((~pauli).sum() + (1.0 - p_id).sum())


def timed(eng, fn, rec, data, shots, seed, meas, ro):
    t0 = time.perf_counter()
    eng.timer_begin()
    fn(rec, data, shots, seed, meas, ro)
    ms = eng.timer_end()
    return ms, (time.perf_counter() - t0) * 1e3


def part_a(args, nm):
    from scipy.stats import halfnorm
    np.random.seed(1984)
    progs = []
    for j, C in enumerate(workloads.REFERENCE_GRAPHS):
        d = sum(2 ** len(c) for c in C)
        for _ in range(args.reps):
            progs.append((j,) + lowered(C, -halfnorm.rvs(loc=0, scale=0.5, size=d), nm))
    engines = {W: _lib.Engine(W) for W in sorted({p[1] for p in progs})}
    for W, eng in engines.items():                                       # warm-up: module load, first launch of each kernel
        j, _, rec, data, meas, ro = next(p for p in progs if p[1] == W)
        eng.noisy_sample(rec, data, args.shots, 1, meas, ro)                # (at full size: the staging buffer grows here)
        eng.noisy_sample_hbm(rec, data, args.shots, 1, meas, ro)
    ms = {}
    for i, (j, W, rec, data, meas, ro) in enumerate(progs):
        eng = engines[W]
        for name, fn in (("lds", eng.noisy_sample), ("hbm", eng.noisy_sample_hbm), ("lds", eng.noisy_sample), ("hbm", eng.noisy_sample_hbm)):
            dev, wall = timed(eng, fn, rec, data, args.shots, 1984 + i, meas, ro)
            ms.setdefault((j, name), []).append((dev, wall))
    for j in range(len(workloads.REFERENCE_GRAPHS)):
        sel = [p for p in progs if p[0] == j]
        lds, hbm = np.array(ms[(j, "lds")]), np.array(ms[(j, "hbm")])
        print(json.dumps({"label": args.label, "part": "a", "graph": j, "W": sel[0][1], "records": int(np.mean([len(p[2]) for p in sel])),
                          "shots": args.shots, "calls": len(lds), "lds_ms": round(float(lds[:, 0].mean()), 4),
                          "lds_ms_min": round(float(lds[:, 0].min()), 4), "hbm_ms": round(float(hbm[:, 0].mean()), 4),
                          "hbm_ms_min": round(float(hbm[:, 0].min()), 4), "hbm_wall_ms": round(float(hbm[:, 1].mean()), 4),
                          "hbm_over_lds": round(float(hbm[:, 0].mean() / lds[:, 0].mean()), 3)}), flush=True)
    for e in engines.values():
        e.close()


def part_b(args, nm):
    for W in sorted(CHAIN_SHOTS):
        cliques = workloads.chain(W // 2)
        theta = workloads.theta_halfnorm(sum(2 ** len(c) for c in cliques))
        w, rec, data, meas, ro = lowered(cliques, theta, nm)
        assert w == W, (w, W)
        rec = rec[:args.records]
        ops = state_ops(rec, data)
        floor_us = 32.0 * 2 ** W / HBM_BYTES_PER_S * 1e6                 # one op of one trajectory at the stream rate
        with _lib.Engine(W) as eng:
            eng.noisy_sample_hbm(rec, data, 4, 1, meas, ro)                # warm-up
            for grid, shots in zip((0, 1), CHAIN_SHOTS[W]):
                eng.set_option("noisy_grid", grid)
                runs = [timed(eng, eng.noisy_sample_hbm, rec, data, shots, 77 + r, meas, ro) for r in range(args.runs)]
                dev = min(r[0] for r in runs)
                us_op = dev * 1e3 / (shots * ops)
                print(json.dumps({"label": args.label, "part": "b", "W": W, "noisy_grid": grid, "shots": shots, "records": len(rec),
                                  "state_ops": round(ops, 1), "ms": round(dev, 3), "wall_ms": round(min(r[1] for r in runs), 3),
                                  "us_per_shot": round(dev * 1e3 / shots, 2), "us_per_shot_op": round(us_op, 4),
                                  "stream_us_per_op": round(floor_us, 4), "fraction_of_stream_rate": round(floor_us / us_op, 4),
                                  "GB_per_s": round(32.0 * 2 ** W * shots * ops / (dev * 1e-3) / 1e9, 1)}), flush=True)
            eng.set_option("noisy_grid", 0)
            # what a shot costs besides its ops: |0..0> written, the final draw (chunk sums by the whole workgroup, then
            # wave 0 cutting the owner's chunk into 64 pieces until one amplitude is left), the word
            shots = CHAIN_SHOTS[W][0]
            dev = min(timed(eng, eng.noisy_sample_hbm, rec[:0], data, shots, 99, meas, ro)[0] for _ in range(3))
            print(json.dumps({"label": args.label, "part": "b", "W": W, "noisy_grid": 0, "shots": shots, "records": 0,
                              "ms": round(dev, 3), "us_per_shot": round(dev * 1e3 / shots, 3),
                              "in_stream_ops": round(dev * 1e3 / shots / floor_us, 2)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="ab")
    ap.add_argument("--shots", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--records", type=int, default=400)
    ap.add_argument("--runs", type=int, default=1)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    nm = ibm_like_model("0.001,0.01", 0.02)
    if "a" in args.part:
        part_a(args, nm)
    if "b" in args.part:
        part_b(args, nm)


if __name__ == "__main__":
    main()
