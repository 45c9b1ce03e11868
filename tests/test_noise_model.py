"""Pauli noise models (qcmrf_amd.noise): Aer conventions, ingest, encoding, the density-matrix reference, and the
backend's noisy path end to end on a numpy engine.  No GPU needed."""
import json
import os

import numpy as np
import pytest

from _density_matrix import NoisyNumpyEngine, chi2_pvalue, density_distribution, _pauli_channel
from oracle import closed_form as cf
from qcmrf_amd import QCMRF, _lib, ingest as ing_mod, ir, noise, program
from qcmrf_amd.backend import QsvBackend
from qcmrf_amd.circuit import QuantumCircuit
from qcmrf_amd.noise import NoiseModel, QuantumError, ReadoutError, depolarizing_error, pauli_error
from qcmrf_amd.transpile import transpile

BASIS = ["cx", "id", "rz", "sx", "x"]
_P1 = {"I": np.eye(2), "X": np.array([[0, 1], [1, 0]]), "Y": np.array([[0, -1j], [1j, 0]]), "Z": np.diag([1, -1])}


def pauli_matrix(label):
    """Qiskit order: the leftmost character is the most significant qubit"""
    m = np.ones((1, 1))
    for c in label:
        m = np.kron(m, _P1[c])
    return m


def superop(err):
    """sum_p P(p) P (x) conj(P): the channel as a matrix on vec(rho)"""
    n = err.num_qubits
    S = 0
    for p, pr in enumerate(err.probabilities):
        P = pauli_matrix(noise.index_to_label(p, n))
        S = S + pr * np.kron(P, P.conj())
    return S


def models_05():
    return json.load(open(os.path.join(os.path.dirname(__file__), "golden", "models_0.5.json")))


def words(ing):
    return [ing.measure.get(c, -1) for c in range(ing.num_clbits)]


def readout_rows(ing):
    return [ing.readout.get(c, (0.0, 0.0)) for c in range(ing.num_clbits)] if ing.readout else None


# ---- Aer conventions ---------------------------------------------------------------------------------------------

def test_depolarizing_tables_and_bounds():
    e = depolarizing_error(0.3, 1)
    assert np.allclose(e.probabilities, [1 - 0.3 * 3 / 4, 0.3 / 4, 0.3 / 4, 0.3 / 4])
    e2 = depolarizing_error(0.2, 2)
    assert e2.probabilities[0] == pytest.approx(1 - 0.2 * 15 / 16)
    assert np.allclose(e2.probabilities[1:], 0.2 / 16)
    assert depolarizing_error(1.0, 1).probabilities == pytest.approx([0.25] * 4)     # completely depolarizing
    assert depolarizing_error(4 / 3, 1).probabilities == pytest.approx([0, 1 / 3, 1 / 3, 1 / 3])   # the upper bound
    depolarizing_error(16 / 15, 2)
    for lam, n in ((-1e-9, 1), (4 / 3 + 1e-9, 1), (16 / 15 + 1e-9, 2), (0.1, 3), (0.1, 0)):
        with pytest.raises(ValueError):
            depolarizing_error(lam, n)


def test_depolarizing_channel_matches_aer_definition():
    """Aer: E(rho) = (1 - lam) rho + lam Tr(rho) I / 2^n"""
    for n, lam in ((1, 0.37), (2, 0.81)):
        d = 2 ** n
        rng = np.random.RandomState(n)
        A = rng.randn(d, d) + 1j * rng.randn(d, d)
        rho = A @ A.conj().T
        rho /= np.trace(rho)
        got = (superop(depolarizing_error(lam, n)) @ rho.reshape(-1)).reshape(d, d)
        assert np.allclose(got, (1 - lam) * rho + lam * np.eye(d) / d)


def test_pauli_error_labels_and_validation():
    e = pauli_error([("XI", 0.25), ("II", 0.75)])
    assert e.probabilities[4] == 0.25 and e.probabilities[0] == 0.75     # X on error qubit 1: x bit 2
    assert pauli_error([("Y", 1.0)]).probabilities[3] == 1.0
    assert pauli_error([("Z", 1.0)]).probabilities[2] == 1.0
    assert pauli_error([("ZY", 1.0)]).to_dict() == {"ZY": 1.0}
    with pytest.raises(ValueError):
        pauli_error([("X", 0.5), ("I", 0.4)])              # does not sum to 1
    with pytest.raises(ValueError):
        pauli_error([("X", 0.5), ("II", 0.5)])             # mixed lengths
    with pytest.raises(ValueError):
        pauli_error([("Q", 1.0)])
    with pytest.raises(ValueError):
        pauli_error([("X", -0.1), ("I", 1.1)])
    pauli_error([("X", 0.5), ("I", 0.5 + 5e-13)])          # within 1e-12


def test_compose_and_tensor_against_channel_matrices():
    rng = np.random.RandomState(7)

    def rand_err(n):
        return QuantumError(rng.dirichlet(np.ones(4 ** n)), n)
    for n in (1, 2):
        a, b = rand_err(n), rand_err(n)
        assert np.allclose(superop(a.compose(b)), superop(b) @ superop(a))
    a, b = rand_err(1), rand_err(1)
    t = a.tensor(b)
    assert t.num_qubits == 2
    want = sum(pa * pb * np.kron(np.kron(pauli_matrix(la), pauli_matrix(lb)), np.kron(pauli_matrix(la), pauli_matrix(lb)).conj())
               for la, pa in zip("IXZY", a.probabilities) for lb, pb in zip("IXZY", b.probabilities))
    # IXZY is the index order of a one-qubit table (x bit, z bit)
    assert [noise.index_to_label(p, 1) for p in range(4)] == list("IXZY")
    assert np.allclose(superop(t), want)
    assert a.expand(b) == b.tensor(a)
    with pytest.raises(ValueError):
        a.compose(rand_err(2))


def test_readout_error_validation():
    r = ReadoutError([[0.97, 0.03], [0.05, 0.95]])
    assert r.flips() == (0.03, 0.05)
    for bad in ([[0.9, 0.2], [0.0, 1.0]], [[1.0, 0.0]], [[1.1, -0.1], [0, 1]], [[[1, 0], [0, 1]]]):
        with pytest.raises(ValueError):
            ReadoutError(bad)


def test_noise_model_precedence_composition_and_refusals():
    nm = NoiseModel()
    assert nm.is_ideal()
    d1 = depolarizing_error(0.1, 1)
    nm.add_all_qubit_quantum_error(d1, ["x", "sx"])
    loc = pauli_error([("Z", 1.0)])
    nm.add_quantum_error(loc, "x", [2])
    assert nm.quantum_error("x", (0,)) is d1
    assert nm.quantum_error("x", (2,)) is loc                      # the local error replaces the all-qubit one
    assert nm.quantum_error("rz", (0,)) is None
    nm.add_all_qubit_quantum_error(pauli_error([("X", 1.0)]), "sx")  # a second error for the same key composes
    assert nm.quantum_error("sx", (0,)) == d1.compose(pauli_error([("X", 1.0)]))
    nm.add_quantum_error(pauli_error([("X", 1.0)]), "x", [2])
    assert nm.quantum_error("x", (2,)) == pauli_error([("Y", 1.0)])
    assert nm.noise_instructions == ["sx", "x"]
    for name in ("measure", "reset", "barrier"):
        with pytest.raises(ValueError):
            nm.add_all_qubit_quantum_error(d1, name)
    with pytest.raises(ValueError):
        nm.add_quantum_error(d1, "cx", [0, 1])                      # arity of the qubit list
    with pytest.raises(TypeError):
        nm.add_all_qubit_quantum_error("depolarizing", "x")
    nm.add_all_qubit_readout_error(ReadoutError([[0.9, 0.1], [0.2, 0.8]]))
    nm.add_readout_error(ReadoutError([[1, 0], [0.5, 0.5]]), [1])
    assert nm.readout_flips(0) == (0.1, 0.2) and nm.readout_flips(1) == (0.0, 0.5)


# ---- ingest and encoding -----------------------------------------------------------------------------------------

def ibm_like(p1=0.01, p2=0.05):
    nm = NoiseModel()
    nm.add_all_qubit_quantum_error(depolarizing_error(p1, 1), ["sx", "x", "id"])
    nm.add_all_qubit_quantum_error(depolarizing_error(p2, 2), ["cx"])
    return nm


def test_ingest_lowered_graph2_one_pauli_per_noisy_gate():
    g = models_05()
    T = transpile(QCMRF(g["GRAPHS"][2], g["THETAS"]["2"][0], with_measurements=True), basis_gates=BASIS)
    names = [ci.operation.name for ci in T.data]
    ing = ing_mod.ingest(T, noise=ibm_like())
    kinds = [o.kind for o in ing.ops]
    assert kinds.count("pauli") == ing.n_pauli == sum(names.count(n) for n in ("sx", "x", "cx"))
    # the device op before every pauli op is the gate it belongs to: never an rz (a diag)
    for i, o in enumerate(ing.ops):
        if o.kind == "pauli":
            assert ing.ops[i - 1].kind in ("u", "x")
            assert len(o.qubits) == (2 if ing.ops[i - 1].ctrls else 1)
            assert tuple(o.qubits) == tuple(ing.ops[i - 1].ctrls) + (ing.ops[i - 1].target,)


def test_ingest_id_takes_its_error_and_cx_label_order():
    qc = QuantumCircuit(2, 2)
    qc.id(0)
    qc.rz(0.3, 1)
    qc.cx(0, 1)
    qc.measure(0, 0)
    qc.measure(1, 1)
    nm = NoiseModel()
    nm.add_all_qubit_quantum_error(pauli_error([("X", 1.0)]), "id")
    nm.add_all_qubit_quantum_error(pauli_error([("XI", 1.0)]), "cx")     # X on qargs[1] = the target
    ing = ing_mod.ingest(qc, noise=nm)
    assert [o.kind for o in ing.ops] == ["pauli", "diag", "x", "pauli"]
    assert ing.ops[0].qubits == (0,)
    assert ing.ops[3].qubits == (0, 1) and ing.ops[3].table[4] == 1.0
    rec, data = program.encode(ing.ops)
    # id puts X on qubit 0 (-> |01>), cx flips qubit 1 (-> |11>), the error's X on the target flips it back: '01'
    dist = density_distribution(rec, data, 2, words(ing))
    assert dist[0b01] == pytest.approx(1.0)


def test_arity_mismatch_raises_at_compile():
    qc = QuantumCircuit(2, 2)
    qc.x(0)
    qc.measure(0, 0)
    nm = NoiseModel()
    nm.add_all_qubit_quantum_error(depolarizing_error(0.1, 2), "x")
    with pytest.raises(ValueError, match="2-qubit error"):
        ing_mod.ingest(qc, noise=nm)


def test_composites_are_unrolled_before_matching():
    """a model on x reaches the X gates inside the AND blocks of a constructed circuit (no error attaches to AND)"""
    qc = QCMRF([[0, 1]], [-0.3, -0.1, -0.7, -0.2], with_measurements=True)
    nm = NoiseModel()
    nm.add_all_qubit_quantum_error(depolarizing_error(0.01, 1), "x")
    ing = ing_mod.ingest(qc, noise=nm)
    n_x = sum(1 for o in ing.ops if o.kind == "x" and not o.ctrls)
    assert ing.n_pauli == n_x > 2                        # the two x of the real-part sandwich and those inside AND


def test_encoding_of_pauli_records():
    e = pauli_error([("XZ", 0.25), ("II", 0.5), ("YY", 0.25)])
    rec, data = program.encode([ir.Op("pauli", qubits=(3, 1), table=e.probabilities)])
    r = rec[0]
    assert int(r["kind"]) == _lib.OP_PAULI == 9
    assert int(r["n"]) == 2 and list(r["qubits"][:2]) == [3, 1]
    cum = data[int(r["data_off"]):int(r["data_off"]) + 16]
    assert np.allclose(np.diff(np.concatenate([[0], cum])), e.probabilities)
    assert cum[-1] == 1.0 and cum[15] == 1.0
    assert (np.diff(cum) >= 0).all()
    assert program.pauli_cumulative([0.5, 0.5 - 1e-17, 0, 0], 1).tolist() == [0.5, 1.0, 1.0, 1.0]


# ---- the density-matrix reference ----------------------------------------------------------------------------------

def test_pauli_channel_matches_kraus_sum():
    rng = np.random.RandomState(3)
    W = 3
    A = rng.randn(8, 8) + 1j * rng.randn(8, 8)
    rho = A @ A.conj().T
    rho /= np.trace(rho)
    probs = rng.dirichlet(np.ones(16))
    qs = (2, 0)
    want = np.zeros_like(rho)
    for p, pr in enumerate(probs):
        P = np.eye(1)
        lab = noise.index_to_label(p, 2)                     # lab[-1] on qs[0], lab[0] on qs[1]
        per = {qs[0]: lab[1], qs[1]: lab[0]}
        for q in reversed(range(W)):
            P = np.kron(P, _P1[per.get(q, "I")])
        want += pr * P @ rho @ P.conj().T
    assert np.allclose(_pauli_channel(rho, qs, probs), want)


def test_density_matrix_zero_noise_equals_closed_form():
    g = models_05()
    zero = NoiseModel()
    zero.add_all_qubit_quantum_error(depolarizing_error(0.0, 1), ["sx", "x", "h"])
    zero.add_all_qubit_quantum_error(depolarizing_error(0.0, 2), ["cx"])
    for j in (1, 4):
        C, th = g["GRAPHS"][j], g["THETAS"][str(j)][3]
        for qc in (QCMRF(C, th, with_measurements=True), transpile(QCMRF(C, th, with_measurements=True), basis_gates=BASIS)):
            ing = ing_mod.ingest(qc, noise=zero)
            assert ing.n_pauli > 0
            rec, data = program.encode(ing.ops)
            dist = density_distribution(rec, data, ing.num_qubits, words(ing))
            assert np.abs(dist - cf.probabilities(C, th)).max() < 1e-12


# ---- the backend's noisy path on a numpy engine --------------------------------------------------------------------

@pytest.fixture
def nbe():
    b = QsvBackend()
    b._engine_factory = lambda n, devices=(0,), rank=None, world_size=None: NoisyNumpyEngine(n, len(devices))
    yield b
    b.close()


def test_backend_noisy_counts_follow_density_matrix(nbe):
    C, th = [[0, 1]], [-0.4, -1.1, -0.2, -0.9]
    T = transpile(QCMRF(C, th, with_measurements=True), basis_gates=BASIS)
    nm = ibm_like(0.02, 0.08)
    nm.add_all_qubit_readout_error(ReadoutError([[0.97, 0.03], [0.05, 0.95]]))
    shots = 4000
    before = NoisyNumpyEngine.calls
    res = nbe.run(T, shots=shots, seed_simulator=11, noise_model=nm).result()
    assert NoisyNumpyEngine.calls == before + 1
    counts = res.get_counts()
    meta = res.metadata(0)
    assert sum(counts.values()) == shots
    assert meta["method"] == "noisy" and meta["n_pauli_ops"] > 0
    for k in ("time_compile", "time_evolve", "time_sample"):
        assert meta[k] >= 0
    ing = ing_mod.ingest(T, noise=nm)
    rec, data = program.encode(ing.ops)
    want = density_distribution(rec, data, ing.num_qubits, words(ing), readout_rows(ing))
    assert chi2_pvalue(counts, want, shots) > 1e-4
    assert chi2_pvalue(counts, cf.probabilities(C, th), shots) < 1e-12


def test_backend_batches_seed_per_circuit(nbe):
    C = [[0, 1]]
    circs = [QCMRF(C, [-0.4, -1.1, -0.2, -0.9], with_measurements=True), QCMRF(C, [-0.1, -0.2, -0.3, -0.4], with_measurements=True)]
    nm = ibm_like()
    res = nbe.run(circs, shots=300, seed_simulator=5, noise_model=nm).result()
    assert [res.metadata(i)["seed_simulator"] for i in range(2)] == [5, 6]
    one = nbe.run(circs[1], shots=300, seed_simulator=6, noise_model=nm).result().get_counts()
    assert res.get_counts(1) == one


def test_backend_without_errors_takes_the_ideal_path(nbe):
    qc = QCMRF([[0, 1]], [-0.4, -1.1, -0.2, -0.9], with_measurements=True)
    base = nbe.run(qc, shots=500, seed_simulator=3).result()
    before = NoisyNumpyEngine.calls
    for model in (None, NoiseModel()):
        res = nbe.run(qc, shots=500, seed_simulator=3, noise_model=model).result()
        assert res.get_counts() == base.get_counts()
        assert "method" not in res.metadata(0)
    assert NoisyNumpyEngine.calls == before


def test_backend_option_plumbing_and_refusals(nbe):
    from qcmrf_amd import get_backend
    nm = ibm_like()
    qc = QCMRF([[0, 1]], [-0.4, -1.1, -0.2, -0.9], with_measurements=True)
    b = get_backend("qasm_simulator", noise_model=nm)
    assert b.options["noise_model"] is nm
    nbe.set_options(noise_model=nm)
    assert nbe.run(qc, shots=50, seed_simulator=1).result().metadata(0)["method"] == "noisy"
    nbe.set_options(noise_model=None)
    with pytest.raises(TypeError):
        nbe.run(qc, shots=10, noise_model={"x": 0.1})
    with pytest.raises(ValueError, match="trajectory"):
        nbe.run(qc, shots=10, noise_model=nm, method="trajectory")

    class TwoRanks:
        world, rank = 2, 0
    with pytest.raises(ValueError, match="limit 1"):
        nbe.run(qc, shots=10, noise_model=nm, comm=TwoRanks())
    wide = QuantumCircuit(14, 1)
    wide.x(13)
    wide.measure(13, 0)
    with pytest.raises(ValueError, match="13"):
        nbe.run(wide, shots=10, noise_model=nm)
    many = QuantumCircuit(2, 65)
    many.x(0)
    many.measure(0, 64)
    with pytest.raises(ValueError, match="64"):
        nbe.run(many, shots=10, noise_model=nm)


def test_run_experiment_model():
    from qcmrf_amd.run_experiment import ibm_like_model
    assert ibm_like_model() is None
    nm = ibm_like_model("0.001,0.02", 0.03)
    assert nm.quantum_error("sx", (4,)) == depolarizing_error(0.001, 1)
    assert nm.quantum_error("id", (0,)) == depolarizing_error(0.001, 1)
    assert nm.quantum_error("cx", (0, 1)) == depolarizing_error(0.02, 2)
    assert nm.quantum_error("rz", (0,)) is None
    assert nm.readout_flips(3) == (0.03, 0.03)
    with pytest.raises(ValueError):
        ibm_like_model("0.1", None)
