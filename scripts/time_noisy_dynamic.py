"""Device time of dynamic record streams (QSV_OP_IF, QSV_OP_RESET): what the kernels that know the two kinds cost, and what
writing a circuit with one shared ancilla and explicit resets costs.

The workload is the lowered chain of 10 variables under the thermal-relaxation model of time_noisy_kraus2.py (product form on
``cx``), 2048 shots, measurements taken in place, with the states on chip and in slots of device memory:

    static     the circuit as QCMRF builds it, ``noisy_measure='in_place'`` (12 live qubits): its own kernels
    forced     the same records through the kernels of qsv_noise_dynamic.hip (engine option ``noisy_dynamic_kernels`` = 1)
    shared     the same chain written the hardware way -- every clique ancilla on one qubit, a ``reset`` behind each ancilla
               measurement --, ``run(dynamic=True)``'s records

    python scripts/time_noisy_dynamic.py [--shots 2048] [--windows 5] [--log profiles/noisy_dynamic.log]

Each call is bracketed by HIP events on the engine's stream (qsv_timer_begin / _end).  A window runs every leg ``--reps``
times, alternating leg by leg in one process, so that drift of the clocks falls on all legs alike; the figure of a leg is the
median over the windows of its mean time per call.  One JSON line per state placement, printed and appended to the log.
``forced/static`` says what the new code objects cost on records the old ones run (the option is a diagnostic and ships off),
``shared/static`` what the explicit resets cost.  The three legs return words of one distribution; ``static`` and ``forced``
the same words."""
import argparse
import json
import os
import sys

import numpy as np

if "PYTHONPATH" not in os.environ:
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from qcmrf_amd import QCMRF, _lib                                        # noqa: E402
from qcmrf_amd.backend import QsvBackend                                 # noqa: E402
from qcmrf_amd.circuit import QuantumCircuit                             # noqa: E402
from qcmrf_amd.noise import NoiseModel, thermal_relaxation_error         # noqa: E402
from qcmrf_amd.transpile import transpile                                # noqa: E402

BASIS = ["cx", "id", "rz", "sx", "x"]
LEGS = ("static", "forced", "shared")


def thermal_model():
    t = thermal_relaxation_error(100e3, 80e3, 300.0)                     # T1 100 us, T2 80 us, cx 300 ns
    nm = NoiseModel()
    nm.add_all_qubit_quantum_error(t.expand(t), ["cx"])
    return nm


def shared_ancilla(T, n):
    """the lowered circuit with every clique ancilla (qubits n + 1 and up) on qubit n + 1 and a reset behind each of their
    measurements"""
    qc = QuantumCircuit(n + 2, T.num_clbits, name="shared_ancilla")
    for ci in T.data:
        qs = [min(T.find_bit(q).index, n + 1) for q in ci.qubits]
        qc.append(ci.operation, qs, [T.find_bit(c).index for c in ci.clbits])
        if ci.operation.name == "measure" and qs[0] == n + 1:
            qc.reset(n + 1)
    return qc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variables", type=int, default=10)
    ap.add_argument("--shots", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--log", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "noisy_dynamic.log"))
    args = ap.parse_args()
    n = args.variables
    cliques = [[i, i + 1] for i in range(n - 1)]
    theta = (-0.3 - 0.05 * (np.arange(4 * (n - 1)) % 11)).tolist()
    T = transpile(QCMRF(cliques, theta, with_measurements=True), basis_gates=BASIS)
    nm = thermal_model()
    lines = []
    for state in ("lds", "hbm"):
        static = QsvBackend._prepare_noisy(T, nm, state, "in_place")
        shared = QsvBackend._prepare_noisy_dynamic(shared_ancilla(T, n), nm, state)
        width = static[8][1]
        assert shared[8][1] == width, "both forms keep n + 2 qubits live"
        sample = {}
        with _lib.Engine(width) as eng:
            fn = eng.noisy_sample_hbm if state == "hbm" else eng.noisy_sample

            def call(leg, shots, seed):
                ing, rec, data, clist, meas, readout = (shared if leg == "shared" else static)[:6]
                eng.set_option("noisy_dynamic_kernels", 1 if leg == "forced" else 0)
                return fn(rec, data, shots, seed, meas, readout if ing.readout else None)

            for leg in LEGS:                                              # warm-up: module load, first launch of each kernel
                sample[leg] = call(leg, 256, 1)
            assert np.array_equal(sample["static"], sample["forced"]), "the forced kernels return other words"
            ms = {leg: [] for leg in LEGS}
            for w in range(args.windows):
                t = {leg: [] for leg in LEGS}
                for r in range(args.reps):
                    for leg in LEGS:
                        eng.timer_begin()
                        call(leg, args.shots, 1984 + r)
                        t[leg].append(eng.timer_end())
                for leg in LEGS:
                    ms[leg].append(float(np.mean(t[leg])))
            eng.set_option("noisy_dynamic_kernels", 0)
        med = {leg: float(np.median(ms[leg])) for leg in LEGS}
        kinds = shared[1]["kind"]
        lines.append(json.dumps({"variables": n, "noisy_state": state, "W": width, "shots": args.shots, "windows": args.windows,
                                 "reps": args.reps, "records": {"static": len(static[1]), "shared": len(shared[1])},
                                 "reset_records": int((kinds == _lib.OP_RESET).sum()), "measure_records": int((kinds == _lib.OP_MEASURE).sum()),
                                 "ms_per_call": {leg: round(med[leg], 4) for leg in LEGS},
                                 "forced/static": round(med["forced"] / med["static"], 4),
                                 "shared/static": round(med["shared"] / med["static"], 4)}))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
