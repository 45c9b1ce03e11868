"""Device time of the density-matrix method (qsv_density_exec and its two channel kernels), HIP events through qsv_timer_*.

    python scripts/time_density.py graphs   [--reps 2] [--shots 10000] [--passes 2]
    python scripts/time_density.py kernels  [--W 13] [--rounds 2]
    python scripts/time_density.py measure  [--W 13] [--windows 5] [--targets 0 5 12] [--kernel 1]

graphs   per graph of the reference experiment: the lowered circuits under the ``--depolarizing 0.001,0.01 --readout 0.02``
         model; ``density_exec`` of each against the 10 000-shot ``noisy_sample`` call of the same program, same build, same
         job.  Every shape is warmed up (one untimed call per width and entry point).
kernels  at W qubits (a vector of 4^W amplitudes): the PAULI kernel for n = 1 and n = 2 and the KRAUS kernel on several
         qubits, each against the same superoperator handed as a dense matrix to ``apply_kq`` (k = 2, 4) on the same bits,
         alternating.  A record's time is the difference between programs of 18 and of 2 equal records, over 16 (the
         program's init pass cancels); 32 B per amplitude over that time, against the 8 TB/s peak.
measure  at W qubits: a MEASURE record through ``density_exec_accept`` (k_dm_measure: 24 B per amplitude) against the same map
         as a KRAUS record of the two operators |0><0| and |1><1| (release: |0><1|) through ``density_exec`` (k_dm_kraus: 32 B),
         on t = 0, 5 and W - 1, with and without release.  A window is one record time as above (18 records minus 2, over
         16); the two routes alternate window by window in one process; the median of the windows is reported with their
         spread.  The outcome is forgotten (weights 1, 1) so that 18 records leave a state: the kernels' work does not
         depend on the weights.  ``--kernel 1`` times k_dm_measure itself on every qubit; without it the record runs as the
         library routes it (below qubit 3 through k_dm_kraus: the two columns then time the same kernel).
One JSON line per measurement."""
import argparse
import json
import os
import sys
import time

import numpy as np

if "PYTHONPATH" not in os.environ:
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from qcmrf_amd import QCMRF, _lib, ingest as ing_mod, ir, program        # noqa: E402
from qcmrf_amd.run_experiment import ibm_like_model                      # noqa: E402
from qcmrf_amd.transpile import transpile                                # noqa: E402
from qcmrf_amd.workloads import REFERENCE_GRAPHS as GRAPHS               # noqa: E402

BASIS = ["cx", "id", "rz", "sx", "x"]
PEAK = 8e12


def graphs(args):
    nm = ibm_like_model("0.001,0.01", 0.02)
    np.random.seed(1984)
    from scipy.stats import halfnorm
    progs = []
    for j, C in enumerate(GRAPHS):
        d = sum(2 ** len(c) for c in C)
        for _ in range(args.reps):
            theta = -halfnorm.rvs(loc=0, scale=0.5, size=d)
            T = transpile(QCMRF(C, theta.tolist(), with_measurements=True), basis_gates=BASIS)
            ing = ing_mod.ingest(T, noise=nm)
            rec, data = program.encode(ing.ops)
            meas = [ing.measure.get(c, -1) for c in range(ing.num_clbits)]
            ro = np.array([ing.readout.get(c, (0.0, 0.0)) for c in range(ing.num_clbits)])
            progs.append((j, ing.num_qubits, rec, data, meas, ro, ing.n_pauli))
    widths = sorted({p[1] for p in progs})
    traj = {W: _lib.Engine(W) for W in widths}
    dens = {W: _lib.Engine(2 * W) for W in widths}
    for W in widths:                                                     # warm-up of every shape
        j, _, rec, data, meas, ro, _ = next(p for p in progs if p[1] == W)
        traj[W].noisy_sample(rec, data, 100, 1, meas, ro)
        dens[W].density_exec(rec, data)
        dens[W].density_sample(100, 1, meas, ro)
    for ps in range(args.passes):
        rows = {}
        for i, (j, W, rec, data, meas, ro, npauli) in enumerate(progs):
            e = dens[W]
            e.timer_begin()
            e.density_exec(rec, data)
            t_exec = e.timer_end()
            e.timer_begin()
            e.density_sample(args.shots, 1984 + i, meas, ro)
            t_samp = e.timer_end()
            e = traj[W]
            e.timer_begin()
            e.noisy_sample(rec, data, args.shots, 1984 + i, meas, ro)
            rows.setdefault(j, []).append((t_exec, t_samp, e.timer_end(), len(rec), npauli))
        for j in sorted(rows):
            r = np.array(rows[j])
            print(json.dumps({"part": "graphs", "pass": ps, "graph": j, "W": next(p[1] for p in progs if p[0] == j), "calls": len(r),
                              "records": int(r[:, 3].mean()), "pauli_ops": int(r[:, 4].mean()),
                              "density_exec_ms": round(float(r[:, 0].mean()), 3), "density_sample_ms": round(float(r[:, 1].mean()), 3),
                              "noisy_sample_ms": round(float(r[:, 2].mean()), 3), "shots": args.shots}), flush=True)
    for e in list(traj.values()) + list(dens.values()):
        e.close()


_P = [np.eye(2), np.array([[0, 1], [1, 0]]), np.array([[1, 0], [0, -1]]), np.array([[0, -1j], [1j, 0]])]   # index x | z << 1


def pauli_superop(probs, n):
    """sum_p probs[p] conj(P) (x) P over (ket bits low, bra bits high); qubit 0 of the record is the low bit of each side"""
    S = np.zeros((4 ** n, 4 ** n), dtype=np.complex128)
    for p, pr in enumerate(probs):
        P = np.eye(1)
        for j in range(n):
            P = np.kron(_P[(p >> (2 * j)) & 3], P)
        S += pr * np.kron(P.conj(), P)
    return S


def kernels(args):
    W = args.W
    rng = np.random.RandomState(13)
    eng = _lib.Engine(2 * W)
    if args.nontemporal is not None:
        eng.set_option("nontemporal", args.nontemporal)
    nbytes = 32.0 * 4 ** W
    head = [ir.op_init((1 << W) - 1)]
    q, _ = np.linalg.qr(rng.randn(4, 2) + 1j * rng.randn(4, 2))
    ks = q.reshape(2, 2, 2)
    p1, p2 = rng.dirichlet(np.ones(4)), rng.dirichlet(np.ones(16))
    cases = []
    for t in (0, 5, W - 1):
        cases.append(("pauli n=1", (t,), ir.Op("pauli", qubits=(t,), table=p1), pauli_superop(p1, 1)))
        cases.append(("kraus m=2", (t,), ir.Op("kraus", qubits=(t,), table=ks), sum(np.kron(k.conj(), k) for k in ks)))
    for qs in ((0, 1), (W - 1, 0), (5, 6)):
        cases.append(("pauli n=2", qs, ir.Op("pauli", qubits=qs, table=p2), pauli_superop(p2, 2)))

    def record_ms(op):
        out = []
        for n in (2, 18):
            rec, data = program.encode(head + [op] * n)
            eng.density_exec(rec, data)                                  # warm-up of this shape
            eng.timer_begin()
            eng.density_exec(rec, data)
            out.append(eng.timer_end())
        return (out[1] - out[0]) / 16.0

    def dense_ms(bits, S):
        eng.apply_kq(bits, S)                                            # warm-up
        eng.timer_begin()
        for _ in range(16):
            eng.apply_kq(bits, S)
        return eng.timer_end() / 16.0

    for rnd in range(args.rounds):
        for name, qs, op, S in cases:
            bits = list(qs) + [x + W for x in qs]
            a = record_ms(op)
            b = dense_ms(bits, S)
            print(json.dumps({"part": "kernels", "round": rnd, "W": W, "record": name, "qubits": list(qs), "kernel_ms": round(a, 4),
                              "kernel_of_peak": round(nbytes / (a * 1e-3) / PEAK, 3), "apply_kq_k": len(bits), "apply_kq_ms": round(b, 4),
                              "apply_kq_of_peak": round(nbytes / (b * 1e-3) / PEAK, 3)}), flush=True)
    eng.close()


def measure(args):
    W = args.W
    eng = _lib.Engine(2 * W)
    if args.nontemporal is not None:
        eng.set_option("nontemporal", args.nontemporal)
    if args.kernel is not None:
        eng.set_option("density_measure_kernel", args.kernel)
    head = [ir.op_init((1 << W) - 1)]

    def window(run, op):
        out = []
        for n in (2, 18):
            rec, data = program.encode(head + [op] * n)
            run(rec, data)                                               # warm-up of this shape
            eng.timer_begin()
            run(rec, data)
            out.append(eng.timer_end())
        return (out[1] - out[0]) / 16.0

    for t in (args.targets or (0, 5, W - 1)):
        for release in (0, 1):
            k1 = np.zeros((2, 2), dtype=np.complex128)
            k1[0 if release else 1, 1] = 1.0
            twin = ir.Op("kraus", qubits=(t,), table=np.array([np.diag([1.0 + 0j, 0.0]), k1]))
            own = ir.Op("measure", target=t, mask=0, vals=(release,), table=(0.0, 0.0))
            a, b = [], []
            for _ in range(args.windows):
                a.append(window(eng.density_exec_accept, own))
                b.append(window(eng.density_exec, twin))
            ma, mb = float(np.median(a)), float(np.median(b))
            print(json.dumps({"part": "measure", "W": W, "t": t, "release": release, "windows": args.windows, "density_measure_kernel": -1 if args.kernel is None else args.kernel,
                              "measure_record_ms": round(ma, 4), "measure_record_min_max": [round(min(a), 4), round(max(a), 4)],
                              "measure_record_of_peak_at_24B": round(24.0 * 4 ** W / (ma * 1e-3) / PEAK, 3),
                              "kraus_twin_ms": round(mb, 4), "kraus_twin_min_max": [round(min(b), 4), round(max(b), 4)],
                              "kraus_twin_of_peak_at_32B": round(32.0 * 4 ** W / (mb * 1e-3) / PEAK, 3), "ratio": round(mb / ma, 3)}), flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=("graphs", "kernels", "measure"))
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--shots", type=int, default=10000)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--W", type=int, default=13)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--kernel", type=int, default=None, help="measure: engine option density_measure_kernel (1: k_dm_measure on every qubit; default: as the library routes the record)")
    ap.add_argument("--targets", type=int, nargs="*", default=None, help="measure: the measured qubits (default 0, 5, W - 1)")
    ap.add_argument("--nontemporal", type=int, default=None, help="engine option of the same name (-1, 0, 1)")
    args = ap.parse_args()
    t0 = time.perf_counter()
    {"graphs": graphs, "kernels": kernels, "measure": measure}[args.part](args)
    print(json.dumps({"part": args.part, "wall_s": round(time.perf_counter() - t0, 1)}), flush=True)


if __name__ == "__main__":
    main()
