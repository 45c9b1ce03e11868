"""The reference's experiment driver (/root/reference/run_experiment.py:1-61) on this engine.

    python -m qcmrf_amd.run_experiment [--scale 0.5] [--shots 10000] [--reps 10] [--outdir .]
                                       [--depolarizing P1,P2] [--readout P] [--t1 US --t2 US --gate-time NS1,NS2]
                                       [--method density_matrix] [--density-measure auto] [--post-select]

Same steps, same files: seed numpy with 1984, draw theta = -halfnorm.rvs(scale) for the 7
hard-coded graphs x REPS, dump ``models_<SCALE>.json``, build the 70 ``QCMRF`` circuits, run them
on the simulator with SHOTS shots, dump ``result_simulation_<SCALE>.json``.  Differences:
``d = sum 2^|C|`` is computed directly (the reference asks the closed-source ``kiopto_native``
for ``len(px.weights(...))``, which is the same number); ``transpile`` is applied only when Qiskit
is importable (the engine ingests the nested circuits directly); the unreachable IBM-hardware
tail (run_experiment.py:63-88) is not reproduced.

With ``--depolarizing P1,P2`` and / or ``--readout P`` the run is noisy instead, with an IBM-like Pauli model: depolarizing
P1 after every ``sx``, ``x`` and ``id``, P2 after every ``cx``, a symmetric readout error P on every qubit.
``--t1 US --t2 US --gate-time NS1,NS2`` adds thermal relaxation (T1 and T2 in microseconds): over NS1 nanoseconds after
every ``sx``, ``x`` and ``id``, over NS2 on both qubits of every ``cx``, each composed with the depolarizing error of
the gate when that is given too.  The circuits are then always lowered to {cx,id,rz,sx,x} (by ``qcmrf_amd.transpile`` when Qiskit is absent) so that those gates exist,
and the counts go to ``result_simulation_noisy_<SCALE>.json``.  ``--noisy-measure in_place`` (or ``auto``) takes the clique
ancillas' measurements when they occur and recycles their qubits: n + 2 live qubits per shot instead of n + m + 1.

``--coherent-cx EPS`` composes the coherent over-rotation exp(-i EPS/2 Z(x)X) of the cross-resonance pulse (Z on the control, X
on the target: ``coherent_unitary_error``, one dense two-qubit Kraus record per ``cx``) onto the ``cx`` error of whatever model
the other noise options build; with no other noise option it is the only error.

``--method density_matrix`` evolves every circuit exactly as a density matrix (noisy or not): the counts are drawn from the
exact distributions, and those are written as well, one ``{bitstring: p}`` per circuit, to ``probs_simulation_<SCALE>.json``
(``probs_simulation_noisy_<SCALE>.json`` for a noisy run).  With ``--post-select``, ``--density-measure in_place`` (or ``auto``)
applies every clique ancilla's accepted measurement where it occurs and recycles the qubit: rho of n + 2 live qubits instead of
n + m + 1, the same exact numbers.

``--post-select`` draws every shot from the branch in which all clique ancillas read 0 (``QCMRF.post_selection()``): the
counts, SHOTS Gibbs samples per circuit with full-width keys, go to ``result_simulation_postselected_<SCALE>.json`` and the
exact success probabilities, one float per circuit, to ``success_simulation_<SCALE>.json``.  Together with the noise options
(or ``--method density_matrix``) the condition becomes the run option ``accept``: noisy attempts are made until SHOTS of them
read 0 on every ancilla (attempts that can no longer be accepted are abandoned on the device; ``--noisy-measure auto`` is
what lets them), the counts go to ``result_simulation_noisy_postselected_<SCALE>.json`` and the success rates to
``success_simulation_noisy_<SCALE>.json``: the estimates (SHOTS - 1) / (attempts - 1), or the exact probabilities with
``--method density_matrix``.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

from .mrf import MAP_MAX_K


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=0.5)
    ap.add_argument("--shots", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--outdir", default=".")
    ap.add_argument("--seed-simulator", type=int, default=None)
    ap.add_argument("--depolarizing", default=None, metavar="P1,P2",
                    help="depolarizing parameter after sx/x/id and after cx (noisy run)")
    ap.add_argument("--readout", type=float, default=None, metavar="P", help="symmetric readout error (noisy run)")
    ap.add_argument("--t1", type=float, default=None, metavar="US", help="T1 in microseconds (noisy run, with --t2 and --gate-time)")
    ap.add_argument("--t2", type=float, default=None, metavar="US", help="T2 in microseconds, at most 2 T1")
    ap.add_argument("--gate-time", default=None, metavar="NS1,NS2", help="duration of sx/x/id and of cx in nanoseconds")
    ap.add_argument("--coherent-cx", type=float, default=None, metavar="EPS",
                    help="coherent over-rotation exp(-i EPS/2 Z(x)X) after every cx, composed onto the cx error of the other options (noisy run)")
    ap.add_argument("--method", default=None, choices=["density_matrix"],
                    help="density_matrix: exact distributions (probs_simulation_*.json) next to the counts drawn from them")
    ap.add_argument("--noisy-measure", default=None, choices=["deferred", "in_place", "auto"],
                    help="noisy run: take every measurement at the end (deferred, the default) or mid-circuit ones when they occur, "
                         "their qubits recycled (in_place; auto: in place iff that makes the per-shot state narrower)")
    ap.add_argument("--density-measure", default=None, choices=["deferred", "auto", "in_place"],
                    help="--method density_matrix: take every measurement at the end (deferred, the default) or apply the mid-circuit ones "
                         "that --post-select fixes where they occur, their qubits recycled (in_place; auto: where possible and narrower)")
    ap.add_argument("--post-select", action="store_true",
                    help="every shot from the branch in which all clique ancillas read 0; also writes the success probabilities "
                         "(exact; estimated from the attempts made when the run is noisy)")
    ap.add_argument("--marginals", action="store_true",
                    help="also write every circuit's clique marginals and success probability (ideal state-vector run, one "
                         "conditioned device pass per circuit) to marginals_simulation_<SCALE>.json")
    ap.add_argument("--map", type=int, default=None, metavar="K",
                    help="also write every circuit's K most probable configurations (exact MAP inference for K = 1), their "
                         "probabilities and the success probability (ideal state-vector run, one conditioned device pass per "
                         "circuit) to map_simulation_<SCALE>.json")
    args = ap.parse_args(argv)
    if args.map is not None and (args.method is not None or any(x is not None for x in (args.depolarizing, args.readout, args.t1, args.t2,
                                                                                        args.gate_time, args.coherent_cx))):
        ap.error("--map reads the ideal state vector and takes no noise option or --method: the most probable outcomes of a noisy "
                 "run are the largest entries of the exact distribution that method=\"density_matrix\" returns (Result.get_probabilities())")
    if args.map is not None and not 1 <= args.map <= MAP_MAX_K:
        ap.error("--map K: K = %d, 1..%d supported" % (args.map, MAP_MAX_K))
    if args.marginals and (args.method is not None or any(x is not None for x in (args.depolarizing, args.readout, args.t1, args.t2,
                                                                                  args.gate_time, args.coherent_cx))):
        ap.error("--marginals reads the ideal state vector and takes no noise option or --method: the marginals of a noisy run "
                 "are sums over the exact distribution that method=\"density_matrix\" returns (Result.get_probabilities())")
    model = ibm_like_model(args.depolarizing, args.readout, args.t1, args.t2, args.gate_time, args.coherent_cx)

    np.random.seed(1984)
    from scipy.stats import halfnorm
    from . import QCMRF, Aer, HAVE_QISKIT
    from .workloads import REFERENCE_GRAPHS as GRAPHS

    THETAS = {}
    for j, C in enumerate(GRAPHS):
        d = sum(2 ** len(c) for c in C)
        for _ in range(args.reps):
            theta = -halfnorm.rvs(loc=0, scale=args.scale, size=d)
            THETAS.setdefault(j, []).append(theta.tolist())
    with open(os.path.join(args.outdir, "models_" + str(args.scale) + ".json"), "w") as f:
        f.write(json.dumps({"GRAPHS": GRAPHS, "THETAS": THETAS}, indent=4))

    CIRCS = [QCMRF(C, THETAS[j][i], with_measurements=True) for j, C in enumerate(GRAPHS) for i in range(args.reps)]
    MODELS = list(CIRCS)
    POST = [qc.post_selection() for qc in CIRCS] if args.post_select else None      # (classical bits: lowering keeps them)
    ACCEPT = POST is not None and (model is not None or args.method is not None)    # no exact conditioned state vector: accept
    if HAVE_QISKIT:                                   # pragma: no cover - Qiskit absent in this image
        from qiskit import transpile
        CIRCS = transpile(CIRCS, basis_gates=['cx', 'id', 'rz', 'sx', 'x'])
    elif model is not None:                           # the model names basis gates: they have to be there
        from .transpile import transpile
        CIRCS = transpile(CIRCS, basis_gates=['cx', 'id', 'rz', 'sx', 'x'])

    simulator = Aer.get_backend('qasm_simulator')
    t0 = time.perf_counter()
    extra = {} if model is None else {"noise_model": model}
    if args.method is not None:
        extra["method"] = args.method
    if args.noisy_measure is not None:
        extra["noisy_measure"] = args.noisy_measure
    if args.density_measure is not None:
        extra["density_measure"] = args.density_measure
    if POST is not None:
        extra["accept" if ACCEPT else "post_select"] = POST
    result = simulator.run(CIRCS, shots=args.shots, seed_simulator=args.seed_simulator, **extra).result()
    counts = result.get_counts()
    dt = time.perf_counter() - t0
    print("%d circuits x %d shots: %.3f s in run().result().get_counts() (%.2f ms per circuit)"
          % (len(CIRCS), args.shots, dt, dt / len(CIRCS) * 1e3), file=sys.stderr)
    noisy = "" if model is None else "noisy_"
    name = "result_simulation_" + noisy + ("postselected_" if POST is not None else "")
    with open(os.path.join(args.outdir, name + str(args.scale) + ".json"), "w") as f:
        f.write(json.dumps(counts, indent=4))
    if POST is not None:
        success = [float(r["metadata"]["accept_probability" if ACCEPT else "post_select_probability"]) for r in result.results]
        with open(os.path.join(args.outdir, "success_simulation_" + noisy + str(args.scale) + ".json"), "w") as f:
            f.write(json.dumps(success, indent=4))
    if args.method == "density_matrix":
        probs = result.get_probabilities()
        name = "probs_simulation_" if model is None else "probs_simulation_noisy_"
        with open(os.path.join(args.outdir, name + str(args.scale) + ".json"), "w") as f:
            f.write(json.dumps(probs if isinstance(probs, list) else [probs], indent=4))
    if args.marginals:
        # the lowered circuit where there is one, conditioned through the model's own classical bits
        rows = [qc.marginals(simulator, circuit=c) for qc, c in zip(MODELS, CIRCS)]
        with open(os.path.join(args.outdir, "marginals_simulation_" + str(args.scale) + ".json"), "w") as f:
            f.write(json.dumps([{"mu": mu.tolist(), "success": float(p)} for mu, p in rows], indent=4))
    if args.map is not None:
        rows = [qc.map_states(simulator, k=args.map, circuit=c) for qc, c in zip(MODELS, CIRCS)]
        with open(os.path.join(args.outdir, "map_simulation_" + str(args.scale) + ".json"), "w") as f:
            f.write(json.dumps([{"x": x.tolist(), "p": p.tolist(), "success": float(ps)} for x, p, ps in rows], indent=4))
    return counts


def cx_over_rotation(eps):
    """exp(-i eps/2 Z(x)X) as a 4 x 4 matrix on the qubits of ``cx(c, t)``: Z on error qubit 0 (c), X on error qubit 1 (t)"""
    zx = np.kron(np.array([[0, 1], [1, 0]], dtype=np.complex128), np.diag([1.0 + 0j, -1.0]))
    return np.cos(0.5 * eps) * np.eye(4) - 1j * np.sin(0.5 * eps) * zx


def ibm_like_model(depolarizing=None, readout=None, t1=None, t2=None, gate_time=None, coherent_cx=None):
    """``--depolarizing P1,P2`` / ``--readout P`` / ``--t1 US --t2 US --gate-time NS1,NS2`` / ``--coherent-cx EPS`` -> a
    NoiseModel (None when none is given).  Thermal relaxation comes first on a gate, the depolarizing error is composed
    after it, the coherent over-rotation of ``cx`` after both."""
    thermal = [x is not None for x in (t1, t2, gate_time)]
    if any(thermal) and not all(thermal):
        raise ValueError("thermal relaxation needs all of --t1, --t2 and --gate-time")
    if depolarizing is None and readout is None and not any(thermal) and coherent_cx is None:
        return None
    from .noise import NoiseModel, ReadoutError, depolarizing_error, thermal_relaxation_error
    nm = NoiseModel()
    if any(thermal):
        times = [float(x) for x in str(gate_time).split(",")]
        if len(times) != 2:
            raise ValueError("--gate-time takes two numbers NS1,NS2, got %r" % (gate_time,))
        one = thermal_relaxation_error(float(t1) * 1e3, float(t2) * 1e3, times[0])
        two = thermal_relaxation_error(float(t1) * 1e3, float(t2) * 1e3, times[1])
        nm.add_all_qubit_quantum_error(one, ["sx", "x", "id"])
        nm.add_all_qubit_quantum_error(two.expand(two), ["cx"])
    if depolarizing is not None:
        parts = [float(x) for x in str(depolarizing).split(",")]
        if len(parts) != 2:
            raise ValueError("--depolarizing takes two numbers P1,P2, got %r" % (depolarizing,))
        nm.add_all_qubit_quantum_error(depolarizing_error(parts[0], 1), ["sx", "x", "id"])
        nm.add_all_qubit_quantum_error(depolarizing_error(parts[1], 2), ["cx"])
    if coherent_cx is not None:
        from .noise import coherent_unitary_error
        nm.add_all_qubit_quantum_error(coherent_unitary_error(cx_over_rotation(float(coherent_cx))), ["cx"])
    if readout is not None:
        p = float(readout)
        nm.add_all_qubit_readout_error(ReadoutError([[1.0 - p, p], [p, 1.0 - p]]))
    return nm


if __name__ == "__main__":
    main()
