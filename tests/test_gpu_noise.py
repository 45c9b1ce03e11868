"""Noisy shots on the MI355X (qsv_noisy_sample, qsv_noise.hip): counts against the exact density-matrix distribution,
determinism of the per-shot random numbers, width limits and the reference experiment with an IBM-like model."""
import json
import os

import numpy as np
import pytest

from _density_matrix import chi2_pvalue, density_distribution, word_distribution
from oracle import closed_form as cf
from qcmrf_amd import QCMRF, _lib, ingest as ing_mod, ir, program
from qcmrf_amd.backend import QsvBackend
from qcmrf_amd.circuit import QuantumCircuit
from qcmrf_amd.noise import NoiseModel, ReadoutError, depolarizing_error, pauli_error
from qcmrf_amd.transpile import transpile

pytestmark = pytest.mark.gpu

BASIS = ["cx", "id", "rz", "sx", "x"]
SHOTS = 20000


@pytest.fixture(scope="module")
def be():
    b = QsvBackend()
    yield b
    b.close()


def models_05():
    return json.load(open(os.path.join(os.path.dirname(__file__), "golden", "models_0.5.json")))


def reference_model(readout=True):
    nm = NoiseModel()
    nm.add_all_qubit_quantum_error(depolarizing_error(0.01, 1), ["sx", "x"])
    nm.add_all_qubit_quantum_error(depolarizing_error(0.05, 2), ["cx"])
    if readout:
        nm.add_all_qubit_readout_error(ReadoutError([[0.97, 0.03], [0.05, 0.95]]))
    return nm


def exact(qc, nm):
    ing = ing_mod.ingest(qc, noise=nm)
    rec, data = program.encode(ing.ops)
    meas = [ing.measure.get(c, -1) for c in range(ing.num_clbits)]
    ro = [ing.readout.get(c, (0.0, 0.0)) for c in range(ing.num_clbits)] if ing.readout else None
    return density_distribution(rec, data, ing.num_qubits, meas, ro)


@pytest.mark.parametrize("j", [0, 1, 2, 4, 5, 6])
def test_lowered_reference_graphs_chi2(be, j):
    g = models_05()
    C, th = g["GRAPHS"][j], g["THETAS"][str(j)][1]
    T = transpile(QCMRF(C, th, with_measurements=True), basis_gates=BASIS)
    nm = reference_model()
    res = be.run(T, shots=SHOTS, seed_simulator=4242 + j, noise_model=nm).result()
    counts = res.get_counts()
    assert sum(counts.values()) == SHOTS
    assert res.metadata(0)["method"] == "noisy"
    assert chi2_pvalue(counts, exact(T, nm), SHOTS) > 1e-4
    assert chi2_pvalue(counts, cf.probabilities(C, th), SHOTS) < 1e-12


def test_constructed_circuit_errors_on_h_and_x(be):
    g = models_05()
    C, th = g["GRAPHS"][2], g["THETAS"]["2"][4]
    qc = QCMRF(C, th, with_measurements=True)
    nm = NoiseModel()
    nm.add_all_qubit_quantum_error(depolarizing_error(0.02, 1), "h")
    nm.add_all_qubit_quantum_error(pauli_error([("X", 0.01), ("Z", 0.02), ("I", 0.97)]), "x")
    res = be.run(qc, shots=SHOTS, seed_simulator=77, noise_model=nm).result()
    counts = res.get_counts()
    assert res.metadata(0)["n_pauli_ops"] > 0
    assert chi2_pvalue(counts, exact(qc, nm), SHOTS) > 1e-4
    assert chi2_pvalue(counts, cf.probabilities(C, th), SHOTS) < 1e-12


def test_zero_probability_errors_follow_closed_form(be):
    g = models_05()
    C, th = g["GRAPHS"][5], g["THETAS"]["5"][2]
    T = transpile(QCMRF(C, th, with_measurements=True), basis_gates=BASIS)
    nm = NoiseModel()
    nm.add_all_qubit_quantum_error(depolarizing_error(0.0, 1), ["sx", "x"])
    nm.add_all_qubit_quantum_error(depolarizing_error(0.0, 2), ["cx"])
    res = be.run(T, shots=SHOTS, seed_simulator=5, noise_model=nm).result()
    assert res.metadata(0)["method"] == "noisy"
    assert chi2_pvalue(res.get_counts(), cf.probabilities(C, th), SHOTS) > 1e-4


def test_readout_only_model_is_the_confusion_of_the_ideal_distribution(be):
    g = models_05()
    C, th = g["GRAPHS"][4], g["THETAS"]["4"][0]
    qc = QCMRF(C, th, with_measurements=True)
    nm = NoiseModel()
    nm.add_all_qubit_readout_error(ReadoutError([[0.9, 0.1], [0.25, 0.75]]))
    nm.add_readout_error(ReadoutError([[1.0, 0.0], [0.0, 1.0]]), [0])
    res = be.run(qc, shots=SHOTS, seed_simulator=8, noise_model=nm).result()
    assert res.metadata(0)["method"] == "noisy" and res.metadata(0)["n_pauli_ops"] == 0
    W = qc.num_qubits
    measured = ing_mod.ingest(qc).measure                # clbit c <- qubit c; clbit n (the work qubit) is never measured
    ro = [(0.1, 0.25) if c in measured and c != 0 else (0.0, 0.0) for c in range(W)]
    want = word_distribution(cf.probabilities(C, th), list(range(W)), ro)
    assert chi2_pvalue(res.get_counts(), want, SHOTS) > 1e-4
    assert chi2_pvalue(res.get_counts(), cf.probabilities(C, th), SHOTS) < 1e-12


def _program(C, th, nm):
    T = transpile(QCMRF(C, th, with_measurements=True), basis_gates=BASIS)
    ing = ing_mod.ingest(T, noise=nm)
    rec, data = program.encode(ing.ops)
    meas = [ing.measure.get(c, -1) for c in range(ing.num_clbits)]
    ro = np.array([ing.readout.get(c, (0.0, 0.0)) for c in range(ing.num_clbits)])
    return ing.num_qubits, rec, data, meas, ro


@pytest.mark.parametrize("cliques", [[[0, 1], [1, 2]], [[0, 1], [1, 2], [2, 3], [3, 4], [4, 5]]])
def test_engine_determinism_prefix_and_grid(cliques):
    W, rec, data, meas, ro = _program(cliques, -np.linspace(0.1, 1.2, sum(2 ** len(c) for c in cliques)), reference_model())
    N = 1500
    with _lib.Engine(W) as eng:
        a = eng.noisy_sample(rec, data, N, 99, meas, ro)
        b = eng.noisy_sample(rec, data, N, 99, meas, ro)
        assert np.array_equal(a, b)
        big = eng.noisy_sample(rec, data, 4 * N, 99, meas, ro)
        assert np.array_equal(big[:N], a)
        for grid in (1, 7, 1000):
            eng.set_option("noisy_grid", grid)
            assert np.array_equal(eng.noisy_sample(rec, data, N, 99, meas, ro), a)
        eng.set_option("noisy_grid", 0)
        other = eng.noisy_sample(rec, data, N, 100, meas, ro)
        assert not np.array_equal(other, a)
        full = eng.noisy_sample(rec, data, 64, 99)                # NULL meas_qubits: the full basis index
        assert full.max() < 2 ** W
        assert (a < 2 ** len(meas)).all()


def test_width_13_runs_and_14_is_refused(be):
    cliques = [[0, 1], [1, 2], [2, 3], [3, 4], [4, 5, 6]]
    theta = (-np.linspace(0.05, 1.5, sum(2 ** len(c) for c in cliques))).tolist()
    qc = QCMRF(cliques, theta, with_measurements=True)
    assert qc.num_qubits == 13
    zero = NoiseModel()
    zero.add_all_qubit_quantum_error(depolarizing_error(0.0, 1), ["h", "x"])
    res = be.run(qc, shots=SHOTS, seed_simulator=13, noise_model=zero).result()
    assert res.metadata(0)["method"] == "noisy" and res.metadata(0)["n_qubits"] == 13
    assert chi2_pvalue(res.get_counts(), cf.probabilities(cliques, theta), SHOTS) > 1e-4
    noisy = NoiseModel()
    noisy.add_all_qubit_quantum_error(depolarizing_error(0.05, 1), ["h", "x"])
    counts = be.run(qc, shots=3000, seed_simulator=13, noise_model=noisy).result().get_counts()
    assert sum(counts.values()) == 3000
    wide = QuantumCircuit(14, 1)
    wide.x(13)
    wide.measure(13, 0)
    with pytest.raises(ValueError, match="13"):
        be.run(wide, shots=10, noise_model=noisy)
    with _lib.Engine(14) as eng:
        rec, data = program.encode([ir.op_x(13)])
        with pytest.raises(ValueError, match="13"):
            eng.noisy_sample(rec, data, 10, 1, [13])


def test_exec_refuses_pauli_and_noisy_refuses_other_kinds():
    rec, data = program.encode([ir.Op("pauli", qubits=(0,), table=np.array([0.5, 0.5, 0.0, 0.0]))])
    with _lib.Engine(3) as eng:
        with pytest.raises(ValueError, match="PAULI"):
            eng.exec(rec, data)
        for op in (ir.op_kq([0, 1], np.eye(4)), ir.op_mux([0], 1, [np.eye(2), np.eye(2)]), ir.Op("swap", a=(0,), b=(1,))):
            r, d = program.encode([op])
            with pytest.raises(RuntimeError, match="-5"):
                eng.noisy_sample(r, d, 10, 1, [0])


def test_reference_experiment_noisy_in_one_run(be):
    from qcmrf_amd.run_experiment import ibm_like_model
    g = models_05()
    circs = [QCMRF(C, g["THETAS"][str(j)][i], with_measurements=True) for j, C in enumerate(g["GRAPHS"]) for i in range(10)]
    T = transpile(circs, basis_gates=BASIS)
    res = be.run(T, shots=10000, seed_simulator=1984, noise_model=ibm_like_model("0.001,0.01", 0.02)).result()
    counts = res.get_counts()
    assert len(counts) == 70
    assert all(sum(c.values()) == 10000 for c in counts)
    assert all(res.metadata(i)["method"] == "noisy" for i in range(70))
