"""Device time of the density-matrix method (qsv_density_exec and its two channel kernels), HIP events through qsv_timer_*.

    python scripts/time_density.py graphs   [--reps 2] [--shots 10000] [--passes 2]
    python scripts/time_density.py kernels  [--W 13] [--rounds 2]

graphs   per graph of the reference experiment: the lowered circuits under the ``--depolarizing 0.001,0.01 --readout 0.02``
         model; ``density_exec`` of each against the 10 000-shot ``noisy_sample`` call of the same program, same build, same
         job.  Every shape is warmed up (one untimed call per width and entry point).
kernels  at W qubits (a vector of 4^W amplitudes): the PAULI kernel for n = 1 and n = 2 and the KRAUS kernel on several
         qubits, each against the same superoperator handed as a dense matrix to ``apply_kq`` (k = 2, 4) on the same bits,
         alternating.  A record's time is the difference between programs of 18 and of 2 equal records, over 16 (the
         program's init pass cancels); 32 B per amplitude over that time, against the 8 TB/s peak.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=("graphs", "kernels"))
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--shots", type=int, default=10000)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--W", type=int, default=13)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--nontemporal", type=int, default=None, help="engine option of the same name (-1, 0, 1)")
    args = ap.parse_args()
    t0 = time.perf_counter()
    (graphs if args.part == "graphs" else kernels)(args)
    print(json.dumps({"part": args.part, "wall_s": round(time.perf_counter() - t0, 1)}), flush=True)


if __name__ == "__main__":
    main()
