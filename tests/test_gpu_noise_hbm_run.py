"""``run(..., noise_model=nm, noisy_state=...)`` end to end on the MI355X: a 14-qubit QCMRF circuit, one qubit more than the
LDS path holds, sampled through the slot path and held to the exact distribution of ``method="density_matrix"`` -- an
independent device path (rho of 14 qubits: 2^28 amplitudes)."""
import numpy as np
import pytest

from _density_matrix import chi2_pvalue
from oracle import closed_form as cf
from qcmrf_amd import QCMRF, workloads
from qcmrf_amd.backend import QsvBackend
from qcmrf_amd.noise import NoiseModel, ReadoutError, amplitude_damping_error, depolarizing_error

pytestmark = pytest.mark.gpu

SHOTS = 4000


@pytest.fixture(scope="module")
def be():
    b = QsvBackend()
    yield b
    b.close()


def model():
    nm = NoiseModel()
    nm.add_all_qubit_quantum_error(depolarizing_error(0.02, 1), "h")                                         # Pauli records
    nm.add_all_qubit_quantum_error(depolarizing_error(0.02, 1).compose(amplitude_damping_error(0.03)), "x")  # Kraus records
    nm.add_all_qubit_readout_error(ReadoutError([[0.97, 0.03], [0.05, 0.95]]))
    return nm


def grid_circuit():
    cliques = workloads.grid(2, 3)
    theta = (-np.linspace(0.05, 1.2, sum(2 ** len(c) for c in cliques))).tolist()
    qc = QCMRF(cliques, theta, with_measurements=True)
    assert qc.num_qubits == 14
    return qc, cf.probabilities(cliques, theta)


def as_array(probs, nbits):
    out = np.zeros(1 << nbits)
    for k, v in probs.items():
        out[int(k.replace(" ", ""), 2)] = v
    return out


def test_14_qubit_qcmrf_follows_the_density_matrix(be):
    (qc, ideal), nm = grid_circuit(), model()
    exact = be.run(qc, shots=0, method="density_matrix", noise_model=nm).result()
    want = as_array(exact.get_probabilities(), qc.num_clbits)
    assert abs(want.sum() - 1.0) < 1e-10
    written = [b for b in range(qc.num_clbits) if want[((np.arange(want.size) >> b) & 1) == 1].sum() > 0]
    assert len(written) == 13
    seen = {}
    for state in ("hbm", "auto"):
        res = be.run(qc, shots=SHOTS, seed_simulator=1414, noise_model=nm, noisy_state=state).result()
        counts, meta = res.get_counts(), res.metadata(0)
        assert meta["method"] == "noisy" and meta["noisy_state"] == "hbm" and meta["n_qubits"] == 14
        assert meta["n_pauli_ops"] > 0 and meta["n_kraus_ops"] > 0 and meta["readout_errors"] > 0
        assert sum(counts.values()) == SHOTS
        p = chi2_pvalue(counts, want, SHOTS)
        # 4000 shots over 2^13 words leave the chi^2 test little power (nearly every cell is pooled), so each written bit's
        # frequency is also held to its exact marginal: within 5 standard deviations of a binomial of SHOTS draws
        got = as_array({k: v / SHOTS for k, v in counts.items()}, qc.num_clbits)
        dev, dev_ideal = [], []
        for b in written:
            one = ((np.arange(want.size) >> b) & 1) == 1
            pb = want[one].sum()
            sigma = np.sqrt(pb * (1.0 - pb) / SHOTS)
            dev.append(abs(got[one].sum() - pb) / sigma)
            dev_ideal.append(abs(got[one].sum() - ideal[one].sum()) / sigma)
        print("HBM RUN noisy_state=%s: chi2 p = %.3g; bit marginals at most %.2f sigma from the density matrix, %.2f from the "
              "ideal distribution" % (state, p, max(dev), max(dev_ideal)))
        assert p > 1e-4
        assert max(dev) <= 5.0
        seen[state] = counts
    assert seen["hbm"] == seen["auto"]                              # the same seed, the same counts
    other = be.run(qc, shots=SHOTS, seed_simulator=1415, noise_model=nm, noisy_state="hbm").result().get_counts()
    assert other != seen["hbm"]
    with pytest.raises(ValueError, match="13"):
        be.run(qc, shots=10, noise_model=nm)


def test_auto_on_5_qubits_is_the_lds_path(be):
    qc = QCMRF([[0, 1, 2]], (-np.linspace(0.1, 1.2, 8)).tolist(), with_measurements=True)
    assert qc.num_qubits == 5
    nm = model()
    base = be.run(qc, shots=SHOTS, seed_simulator=55, noise_model=nm).result()
    auto = be.run(qc, shots=SHOTS, seed_simulator=55, noise_model=nm, noisy_state="auto").result()
    assert base.metadata(0)["noisy_state"] == "lds" and auto.metadata(0)["noisy_state"] == "lds"
    assert auto.get_counts() == base.get_counts()
    hbm = be.run(qc, shots=SHOTS, seed_simulator=55, noise_model=nm, noisy_state="hbm").result()
    assert hbm.metadata(0)["noisy_state"] == "hbm" and sum(hbm.get_counts().values()) == SHOTS
