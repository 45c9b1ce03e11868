"""Kraus channels on the MI355X through ``run()``: counts against the exact density-matrix distribution, and the effect
the channels exist for -- relaxation towards |0> inflates the all-ancillas-zero success rate, which no Pauli model does."""
import pytest

import _kraus_cases as kc
import _noise_exact_cases as nc
from _density_matrix import chi2_pvalue
from _kraus_reference import kraus_density_distribution
from oracle import closed_form as cf
from qcmrf_amd import QCMRF, ingest as ing_mod, program
from qcmrf_amd.backend import QsvBackend
from qcmrf_amd.noise import NoiseModel, ReadoutError, amplitude_damping_error, thermal_relaxation_error
from qcmrf_amd.transpile import transpile

pytestmark = pytest.mark.gpu

SHOTS = 20000


@pytest.fixture(scope="module")
def be():
    b = QsvBackend()
    yield b
    b.close()


def exact(qc, nm):
    ing = ing_mod.ingest(qc, noise=nm)
    rec, data = program.encode(ing.ops)
    meas = [ing.measure.get(c, -1) for c in range(ing.num_clbits)]
    ro = [ing.readout.get(c, (0.0, 0.0)) for c in range(ing.num_clbits)] if ing.readout else None
    return kraus_density_distribution(rec, data, ing.num_qubits, meas, ro)


def check(be, qc, nm, C, th, seed):
    res = be.run(qc, shots=SHOTS, seed_simulator=seed, noise_model=nm).result()
    counts = res.get_counts()
    meta = res.metadata(0)
    assert sum(counts.values()) == SHOTS and meta["method"] == "noisy" and meta["n_kraus_ops"] > 0
    p_fit, p_ideal = chi2_pvalue(counts, exact(qc, nm), SHOTS), chi2_pvalue(counts, cf.probabilities(C, th), SHOTS)
    print("KRAUS chi2: p(density matrix) = %.3g, p(ideal closed form) = %.3g, %d kraus ops" % (p_fit, p_ideal, meta["n_kraus_ops"]))
    assert p_fit > 1e-4
    assert p_ideal < 1e-12
    return meta


def test_damping_only_model_on_a_constructed_circuit(be):
    g = nc.models_05()
    C, th = g["GRAPHS"][0], g["THETAS"]["0"][3]
    qc = QCMRF(C, th, with_measurements=True)
    nm = NoiseModel()
    nm.add_all_qubit_quantum_error(amplitude_damping_error(0.2), ["h", "x"])
    meta = check(be, qc, nm, C, th, 501)
    assert meta["n_pauli_ops"] == 0


def test_thermal_model_on_a_lowered_reference_graph(be):
    g = nc.models_05()
    C, th = g["GRAPHS"][1], g["THETAS"]["1"][2]
    T = transpile(QCMRF(C, th, with_measurements=True), basis_gates=nc.BASIS)
    one, two = thermal_relaxation_error(20e3, 30e3, 200.0), thermal_relaxation_error(20e3, 30e3, 1500.0)
    nm = NoiseModel()
    nm.add_all_qubit_quantum_error(one, ["sx", "x", "id"])
    nm.add_all_qubit_quantum_error(two.expand(two), ["cx"])
    nm.add_all_qubit_readout_error(ReadoutError([[0.97, 0.03], [0.05, 0.95]]))
    meta = check(be, T, nm, C, th, 502)
    assert meta["n_pauli_ops"] == 0 and meta["readout_errors"] > 0


def test_thermal_composed_with_depolarizing_on_cx(be):
    g = nc.models_05()
    C, th = g["GRAPHS"][4], g["THETAS"]["4"][1]
    T = transpile(QCMRF(C, th, with_measurements=True), basis_gates=nc.BASIS)
    meta = check(be, T, kc.thermal_model(), C, th, 503)
    names = [ci.operation.name for ci in T.data]
    assert meta["n_pauli_ops"] == names.count("cx")                 # the two-qubit depolarizing table behind the product


def test_damping_inflates_the_success_rate_where_its_pauli_twirl_lowers_it(be):
    T, n = kc.success_circuit()
    damp, twirl = kc.success_models(0.2)
    rates = []
    for nm, seed in ((damp, 601), (twirl, 602)):
        counts = be.run(T, shots=SHOTS, seed_simulator=seed, noise_model=nm).result().get_counts()
        assert chi2_pvalue(counts, exact(T, nm), SHOTS) > 1e-4
        rates.append(kc.success_rate(counts, n))
    print("KRAUS success rate: damping %.4f, Pauli twirl %.4f" % tuple(rates))
    assert rates[0] > rates[1]
