"""One-qubit Kraus channels on the host: the model (qcmrf_amd.noise), ingest, the encoded record, and ``run()`` end to
end on a numpy stand-in engine.  The one test here that needs the device (``qsv_exec`` refusing the record) is marked."""
import numpy as np
import pytest

from _density_matrix import chi2_pvalue
from _kraus_reference import KrausNumpyEngine, kraus_density_distribution, kraus_of_record
from qcmrf_amd import QCMRF, _lib, ingest as ing_mod, ir, program
from qcmrf_amd.backend import QsvBackend
from qcmrf_amd.circuit import QuantumCircuit
from qcmrf_amd.noise import (NoiseModel, amplitude_damping_error, depolarizing_error, kraus_error, pauli_error,
                             phase_amplitude_damping_error, phase_damping_error, reset_error, thermal_relaxation_error)
from qcmrf_amd.transpile import transpile

BASIS = ["cx", "id", "rz", "sx", "x"]
I2 = np.eye(2, dtype=np.complex128)
X = np.array([[0, 1], [1, 0]], dtype=np.complex128)
Z = np.diag([1.0, -1.0]).astype(np.complex128)
S_ID = np.eye(4)
S_R0 = np.array([[1, 0, 0, 1], [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]], dtype=np.float64)     # rho -> |0><0| tr rho
S_R1 = S_R0[::-1].copy()                                                                        # rho -> |1><1| tr rho
S_Z = np.kron(Z.conj(), Z)


def superop_of(ks):
    """column-stacking: rho_ij at index i + 2j, S = sum conj(K) (x) K"""
    return sum(np.kron(k.conj(), k) for k in ks)


def apply_superop(S, rho):
    d = rho.shape[0]
    return (S @ rho.T.ravel()).reshape(d, d).T


def rand_rho(rng, d=2):
    a = rng.randn(d, d) + 1j * rng.randn(d, d)
    rho = a @ a.conj().T
    return rho / np.trace(rho)


def damping_set(a, b, p1):
    c = np.sqrt(1 - a - b)
    return [np.sqrt(1 - p1) * np.diag([1, c]), np.sqrt(1 - p1) * np.sqrt(a) * np.array([[0, 1], [0, 0]]),
            np.sqrt(1 - p1) * np.sqrt(b) * np.diag([0, 1]), np.sqrt(p1) * np.diag([c, 1]),
            np.sqrt(p1) * np.sqrt(a) * np.array([[0, 0], [1, 0]]), np.sqrt(p1) * np.sqrt(b) * np.diag([1, 0])]


# ---- constructors ---------------------------------------------------------------------------------------------------------

def test_kraus_error_keeps_operators_and_refuses_non_channels():
    ks = [np.diag([1.0, np.sqrt(0.7)]), np.sqrt(0.3) * np.array([[0, 1], [0, 0]])]
    e = kraus_error(ks)
    assert e.num_qubits == 1 and not e.is_ideal()
    got = e.kraus()
    assert len(got) == 2 and all(np.array_equal(g, k) for g, k in zip(got, ks))      # as given, in order
    (kind, qs, stack), = e.terms()
    assert kind == "kraus" and qs == (0,) and stack.shape == (2, 2, 2) and np.array_equal(stack[1], ks[1])
    with pytest.raises(ValueError, match="Pauli"):
        e.probabilities
    with pytest.raises(ValueError, match="identity"):
        kraus_error([np.diag([1.0, 0.5])])                                          # not trace preserving
    with pytest.raises(ValueError, match="identity"):
        kraus_error([I2, 1e-5 * X])                                                 # off by 1e-10 > 1e-12
    with pytest.raises(ValueError):
        kraus_error([])
    with pytest.raises(ValueError, match="2 x 2"):
        kraus_error([np.eye(3)])
    with pytest.raises(ValueError, match="two-qubit Kraus"):
        kraus_error([np.eye(4)])
    assert kraus_error([I2]).is_ideal()
    assert kraus_error([np.diag([1.0, 1j])]) != kraus_error([I2])


def test_more_than_four_operators_are_reduced_to_the_canonical_set():
    ks = damping_set(0.2, 0.3, 0.25)
    e = kraus_error(ks)
    got = e.kraus()
    assert len(got) <= 4
    assert np.allclose(superop_of(got), superop_of(ks), atol=1e-14)
    lam = [np.trace(k.conj().T @ k).real for k in got]
    assert all(a >= b - 1e-15 for a, b in zip(lam, lam[1:]))                        # descending eigenvalues
    assert e == phase_amplitude_damping_error(0.2, 0.3, 0.25)
    assert len(phase_amplitude_damping_error(0.2, 0.3, 0.25).kraus()) <= 4


def test_damping_constructors_against_their_closed_form():
    for a, b, p1 in ((0.2, 0.3, 0.25), (0.5, 0.0, 0.0), (0.0, 0.4, 0.0), (1.0, 0.0, 0.0), (0.3, 0.7, 1.0)):
        want = superop_of(damping_set(a, b, p1))
        assert np.allclose(phase_amplitude_damping_error(a, b, p1).superoperator(), want, atol=1e-14)
    assert amplitude_damping_error(0.3, 0.1) == phase_amplitude_damping_error(0.3, 0.0, 0.1)
    assert phase_damping_error(0.3) == phase_amplitude_damping_error(0.0, 0.3)
    ad = amplitude_damping_error(0.3).kraus()
    assert len(ad) == 2 and np.allclose(ad[0], np.diag([1, np.sqrt(0.7)])) and np.allclose(ad[1], np.sqrt(0.3) * np.array([[0, 1], [0, 0]]))
    assert amplitude_damping_error(0.0).is_ideal()
    for bad in ((-0.1, 0.0, 0.0), (0.6, 0.5, 0.0), (0.1, 0.1, 1.5), (1.2, 0.0, 0.0)):
        with pytest.raises(ValueError):
            phase_amplitude_damping_error(*bad)


def test_reset_error_closed_form_and_validation():
    S = reset_error(0.2, 0.1).superoperator()
    assert np.allclose(S, 0.7 * S_ID + 0.2 * S_R0 + 0.1 * S_R1, atol=1e-15)
    rho = rand_rho(np.random.RandomState(1))
    assert np.allclose(apply_superop(reset_error(1.0).superoperator(), rho), np.diag([1.0, 0.0]))
    assert np.allclose(apply_superop(reset_error(0.0, 1.0).superoperator(), rho), np.diag([0.0, 1.0]))
    assert reset_error(0.0).is_ideal()
    for bad in ((-0.1, 0.0), (0.7, 0.4), (0.0, -1e-3)):
        with pytest.raises(ValueError):
            reset_error(*bad)


@pytest.mark.parametrize("t1, t2, time, p1", [(100.0, 80.0, 10.0, 0.0), (100.0, 100.0, 35.0, 0.2), (50.0, 20.0, 5.0, 1.0),
                                              (np.inf, 70.0, 10.0, 0.3)])
def test_thermal_relaxation_below_t1_is_the_mixture_of_identity_z_and_resets(t1, t2, time, p1):
    e1, e2 = np.exp(-time / t1), np.exp(-time / t2)
    pr, p0 = 1.0 - e1, 1.0 - p1
    pz = (1.0 - pr) * (1.0 - e2 / e1) / 2.0
    pr0, pr1 = p0 * pr, p1 * pr
    want = (1.0 - pz - pr0 - pr1) * S_ID + pz * S_Z + pr0 * S_R0 + pr1 * S_R1
    err = thermal_relaxation_error(t1, t2, time, p1)
    assert np.allclose(err.superoperator(), want, atol=1e-14)
    closed = np.array([[1 - p1 * pr, 0, 0, p0 * pr], [0, e2, 0, 0], [0, 0, e2, 0], [p1 * pr, 0, 0, 1 - p0 * pr]])
    assert np.allclose(err.superoperator(), closed, atol=1e-14)
    ks = err.kraus()
    assert len(ks) <= 4 and np.allclose(sum(k.conj().T @ k for k in ks), I2, atol=1e-13)
    assert np.allclose(superop_of(ks), closed, atol=1e-13)                         # another Kraus set, the same map


@pytest.mark.parametrize("t1, t2, time, p1", [(100.0, 150.0, 10.0, 0.0), (100.0, 200.0, 50.0, 0.3), (30.0, 45.0, 3.0, 1.0)])
def test_thermal_relaxation_above_t1_is_still_cptp(t1, t2, time, p1):
    err = thermal_relaxation_error(t1, t2, time, p1)
    e2, pr, p0 = np.exp(-time / t2), 1.0 - np.exp(-time / t1), 1.0 - p1
    closed = np.array([[1 - p1 * pr, 0, 0, p0 * pr], [0, e2, 0, 0], [0, 0, e2, 0], [p1 * pr, 0, 0, 1 - p0 * pr]])
    assert np.allclose(err.superoperator(), closed, atol=1e-14)
    ks = err.kraus()
    assert 1 <= len(ks) <= 4
    assert np.allclose(sum(k.conj().T @ k for k in ks), I2, atol=1e-13)            # trace preserving
    assert np.allclose(superop_of(ks), closed, atol=1e-13)                         # completely positive: it HAS a Kraus form


def test_thermal_relaxation_validation():
    for bad in ((0.0, 1.0, 1.0), (1.0, -1.0, 1.0), (1.0, 2.5, 1.0), (1.0, 1.0, -1.0), (1.0, 1.0, 1.0, 1.5)):
        with pytest.raises(ValueError):
            thermal_relaxation_error(*bad)
    assert thermal_relaxation_error(100.0, 200.0, 0.0).is_ideal()
    assert thermal_relaxation_error(np.inf, np.inf, 10.0).is_ideal()


# ---- compose, tensor, equality ------------------------------------------------------------------------------------------------

def test_compose_multiplies_superoperators_and_lifts_pauli_tables():
    a, t = amplitude_damping_error(0.3), thermal_relaxation_error(100.0, 120.0, 20.0, 0.1)
    d = depolarizing_error(0.2, 1)
    assert np.allclose(a.compose(t).superoperator(), t.superoperator() @ a.superoperator(), atol=1e-14)   # t AFTER a
    assert np.allclose(d.compose(a).superoperator(), a.superoperator() @ d.superoperator(), atol=1e-14)
    assert np.allclose(a.compose(d).superoperator(), d.superoperator() @ a.superoperator(), atol=1e-14)
    assert a.compose(t) != t.compose(a)
    lifted = sum(p * np.kron(P.conj(), P) for p, P in zip(d.probabilities, (I2, X, Z, 1j * X @ Z)))
    assert np.allclose(d.superoperator(), lifted, atol=1e-15)
    assert len(a.compose(t).kraus()) <= 4
    with pytest.raises(ValueError):
        a.compose(depolarizing_error(0.1, 2))


def test_pauli_with_pauli_is_still_a_pauli_table():
    p, q = pauli_error([("X", 0.1), ("I", 0.9)]), depolarizing_error(0.2, 1)
    c = p.compose(q)
    assert c.is_pauli() and c.probabilities.shape == (4,) and abs(c.probabilities.sum() - 1) < 1e-15
    t2 = p.tensor(q)
    assert t2.is_pauli() and t2.probabilities.shape == (16,)
    assert np.allclose(t2.probabilities, np.outer(p.probabilities, q.probabilities).ravel())
    (kind, qs, table), = c.terms()
    assert kind == "pauli" and qs == (0,) and table is c.probabilities
    # a composed channel that happens to be a Pauli channel is handed to the device as a Pauli table
    z = phase_damping_error(0.2).compose(depolarizing_error(0.1, 1))
    (kind, qs, table), = z.terms()
    assert kind == "pauli" and abs(table.sum() - 1) < 1e-15


def test_tensor_and_expand_against_kronecker_products():
    rng = np.random.RandomState(5)
    a, t = amplitude_damping_error(0.3, 0.1), thermal_relaxation_error(100.0, 150.0, 20.0)
    rho = rand_rho(rng, 4)

    def kron_channel(k1, k0):                                       # k1 on error qubit 1 (the high bit), k0 on qubit 0
        return sum(np.kron(x, y) @ rho @ np.kron(x, y).conj().T for x in k1 for y in k0)

    at = a.tensor(t)                                                # t on error qubit 0, a on error qubit 1
    assert at.num_qubits == 2 and not at.is_pauli()
    assert [(k, qs) for k, qs, _ in at.terms()] == [("kraus", (0,)), ("kraus", (1,))]
    assert np.allclose(apply_superop(at.superoperator(), rho), kron_channel(a.kraus(), t.kraus()), atol=1e-13)
    assert a.expand(t) == t.tensor(a) and a.expand(t) != a.tensor(t)
    assert np.allclose(apply_superop(a.expand(t).superoperator(), rho), kron_channel(t.kraus(), a.kraus()), atol=1e-13)
    mixed = depolarizing_error(0.2, 1).tensor(a)                    # a Pauli factor meets a non-Pauli one: lifted
    assert [(k, qs) for k, qs, _ in mixed.terms()] == [("kraus", (0,)), ("pauli", (1,))]
    assert np.allclose(apply_superop(mixed.superoperator(), rho), kron_channel(depolarizing_error(0.2, 1).kraus(), a.kraus()), atol=1e-13)
    with pytest.raises(ValueError):
        at.tensor(a)
    with pytest.raises(ValueError):
        at.kraus()


def test_two_qubit_compose_concatenates_and_merges_terms():
    t, a = thermal_relaxation_error(100.0, 150.0, 20.0), amplitude_damping_error(0.2)
    d2 = depolarizing_error(0.1, 2)
    e = t.expand(t).compose(d2)
    assert [(k, qs) for k, qs, _ in e.terms()] == [("kraus", (0,)), ("kraus", (1,)), ("pauli", (0, 1))]
    assert e.terms()[2][2] is d2.probabilities
    assert np.allclose(e.superoperator(), d2.superoperator() @ t.expand(t).superoperator(), atol=1e-13)
    # adjacent terms of one shape on the same qubits merge
    ee = e.compose(d2).compose(a.tensor(a)).compose(t.expand(a))
    shape = [(k, qs) for k, qs, _ in ee.terms()]
    assert shape == [("kraus", (0,)), ("kraus", (1,)), ("pauli", (0, 1)), ("kraus", (0,)), ("kraus", (1,))]
    assert np.allclose(ee.terms()[2][2], d2.compose(d2).probabilities)
    assert np.allclose(superop_of(ee.terms()[3][2]), t.superoperator() @ a.superoperator(), atol=1e-13)    # qubit 0: a then t
    assert np.allclose(superop_of(ee.terms()[4][2]), a.superoperator() @ a.superoperator(), atol=1e-13)
    assert d2.compose(t.expand(t)) != e                             # the order of the terms is the order of the channels
    assert not e.is_ideal() and thermal_relaxation_error(1.0, 1.0, 0.0).tensor(reset_error(0.0)).is_ideal()


def test_equality_is_by_superoperator_not_by_kraus_list():
    ks = [np.diag([1.0, np.sqrt(0.7)]), np.sqrt(0.3) * np.array([[0, 1], [0, 0]])]
    u = np.array([[1, 1], [1, -1]]) / np.sqrt(2.0)                  # another Kraus set of the same map
    mixed = [u[0, 0] * ks[0] + u[0, 1] * ks[1], u[1, 0] * ks[0] + u[1, 1] * ks[1]]
    assert kraus_error(ks) == kraus_error(mixed) == amplitude_damping_error(0.3)
    assert kraus_error(ks) != amplitude_damping_error(0.31)
    assert kraus_error([np.sqrt(0.9) * I2, np.sqrt(0.1) * X]) == pauli_error([("X", 0.1), ("I", 0.9)])
    assert pauli_error([("X", 0.1), ("I", 0.9)]) == kraus_error([np.sqrt(0.9) * I2, np.sqrt(0.1) * X])
    assert (amplitude_damping_error(0.3) == "x") is False


# ---- the model and ingest -------------------------------------------------------------------------------------------------------

def test_noise_model_composes_and_still_refuses_measure_reset_barrier():
    t = thermal_relaxation_error(100.0, 80.0, 10.0)
    nm = NoiseModel()
    nm.add_all_qubit_quantum_error(t, ["sx", "x"])
    nm.add_all_qubit_quantum_error(depolarizing_error(0.1, 1), ["sx"])
    assert nm.quantum_error("sx", (3,)) == t.compose(depolarizing_error(0.1, 1))
    assert nm.quantum_error("x", (3,)) == t and not nm.is_ideal()
    for name in ("measure", "reset", "barrier"):
        with pytest.raises(ValueError):
            nm.add_all_qubit_quantum_error(t, name)
        with pytest.raises(ValueError):
            nm.add_quantum_error(t, name, [0])
    with pytest.raises(ValueError):
        nm.add_quantum_error(t.tensor(t), "cx", [0])


@pytest.mark.parametrize("ctrl, tgt", [(0, 2), (2, 0)])
def test_ingest_emits_product_plus_pauli_terms_on_cx_in_order(ctrl, tgt):
    a0, a1 = amplitude_damping_error(0.2), reset_error(0.1, 0.05)
    d2 = depolarizing_error(0.1, 2)
    err = a1.tensor(a0).compose(d2)                                 # a0 on error qubit 0 = qargs[0] = the control
    nm = NoiseModel()
    nm.add_all_qubit_quantum_error(err, "cx")
    nm.add_all_qubit_quantum_error(thermal_relaxation_error(100.0, 80.0, 10.0), "x")
    qc = QuantumCircuit(3, 3)
    qc.x(1)
    qc.cx(ctrl, tgt)
    qc.measure([0, 1, 2], [0, 1, 2])
    ing = ing_mod.ingest(qc, noise=nm)
    kinds = [(o.kind, tuple(o.qubits) if o.kind in ("pauli", "kraus") else None) for o in ing.ops]
    assert kinds == [("x", None), ("kraus", (1,)), ("x", None), ("kraus", (ctrl,)), ("kraus", (tgt,)), ("pauli", (ctrl, tgt))]
    assert np.allclose(superop_of(ing.ops[3].table), a0.superoperator(), atol=1e-14)
    assert np.allclose(superop_of(ing.ops[4].table), a1.superoperator(), atol=1e-14)
    assert ing.ops[5].table is d2.probabilities
    assert ing.n_kraus == 3 and ing.n_pauli == 1
    assert ing.ops[3].support() == (ctrl,)


def test_encoded_kraus_record_round_trips():
    ks = np.array(thermal_relaxation_error(100.0, 150.0, 20.0, 0.2).kraus())
    rec, data = program.encode([ir.op_x(0), ir.Op("kraus", qubits=(5,), table=ks), ir.Op("kraus", qubits=(2,), table=np.array([X]))])
    assert _lib.OP_PAULI == 9 and _lib.OP_KRAUS == 10 and rec.dtype.itemsize == 168
    r = rec[1]
    assert r["kind"] == _lib.OP_KRAUS and r["n"] == 1 and r["qubits"][0] == 5 and r["vals"][0] == len(ks)
    K, E = kraus_of_record(data, int(r["data_off"]), len(ks))
    assert np.array_equal(K, ks)
    for k in range(len(ks)):
        e = ks[k].conj().T @ ks[k]
        assert np.allclose(E[k], [e[0, 0].real, e[1, 1].real, e[0, 1].real, e[0, 1].imag], atol=1e-16)
    assert np.allclose(E[:, :2].sum(axis=0), 1.0) and np.allclose(E[:, 2:].sum(axis=0), 0.0, atol=1e-15)
    r = rec[2]
    assert r["vals"][0] == 1 and r["qubits"][0] == 2
    K, E = kraus_of_record(data, int(r["data_off"]), 1)
    assert np.array_equal(K[0], X) and np.array_equal(E[0], [1.0, 1.0, 0.0, 0.0])
    with pytest.raises(ValueError):
        program.encode([ir.Op("kraus", qubits=(0,), table=np.array([I2] * 5))])
    with pytest.raises(ValueError):
        program.encode([ir.Op("kraus", qubits=(0,), table=np.array([0.5 * I2]))])


@pytest.mark.gpu
def test_exec_refuses_kraus_records():
    rec, data = program.encode([ir.Op("kraus", qubits=(0,), table=np.array(amplitude_damping_error(0.3).kraus()))])
    with _lib.Engine(3) as eng:
        with pytest.raises(ValueError, match="KRAUS"):
            eng.exec(rec, data)
        got = eng.noisy_sample(rec, data, 16, 1)                    # the same record runs as a noisy shot
        assert got.shape == (16,) and not got.any()


# ---- run() end to end on the numpy stand-in engine ------------------------------------------------------------------------------

@pytest.fixture()
def kbe():
    b = QsvBackend()
    b._engine_factory = lambda n, devices=(0,), rank=None, world_size=None: KrausNumpyEngine(n, len(devices))
    yield b
    b.close()


def exact(qc, nm):
    ing = ing_mod.ingest(qc, noise=nm)
    rec, data = program.encode(ing.ops)
    meas = [ing.measure.get(c, -1) for c in range(ing.num_clbits)]
    ro = [ing.readout.get(c, (0.0, 0.0)) for c in range(ing.num_clbits)] if ing.readout else None
    return kraus_density_distribution(rec, data, ing.num_qubits, meas, ro)


def test_run_with_thermal_model_follows_the_density_matrix(kbe):
    from qcmrf_amd.run_experiment import ibm_like_model
    C, th = [[0, 1]], [-0.4, -1.1, -0.2, -0.9]
    T = transpile(QCMRF(C, th, with_measurements=True), basis_gates=BASIS)
    nm = ibm_like_model("0.01,0.05", 0.03, t1=20.0, t2=30.0, gate_time="200,1500")
    shots = 20000
    res = kbe.run(T, shots=shots, seed_simulator=12, noise_model=nm).result()
    meta = res.metadata(0)
    assert meta["method"] == "noisy" and meta["n_kraus_ops"] > 0 and meta["n_pauli_ops"] > 0
    names = [ci.operation.name for ci in T.data]
    n1, n2 = sum(names.count(g) for g in ("sx", "x", "id")), names.count("cx")
    assert meta["n_kraus_ops"] == n1 + 2 * n2 and meta["n_pauli_ops"] == n2       # 1q: thermal and depolarizing merge into one channel
    counts = res.get_counts()
    assert sum(counts.values()) == shots
    assert chi2_pvalue(counts, exact(T, nm), shots) > 1e-4
    from oracle import closed_form as cf
    assert chi2_pvalue(counts, cf.probabilities(C, th), shots) < 1e-12


def test_run_experiment_thermal_options():
    from qcmrf_amd.run_experiment import ibm_like_model
    assert ibm_like_model() is None
    nm = ibm_like_model(t1=100.0, t2=80.0, gate_time="35,300")
    one, two = thermal_relaxation_error(100e3, 80e3, 35.0), thermal_relaxation_error(100e3, 80e3, 300.0)
    for g in ("sx", "x", "id"):
        assert nm.quantum_error(g, (0,)) == one
    assert nm.quantum_error("cx", (0, 1)) == two.expand(two)
    assert nm.readout_flips(0) is None
    both = ibm_like_model("0.001,0.01", 0.02, 100.0, 80.0, "35,300")
    assert both.quantum_error("sx", (1,)) == one.compose(depolarizing_error(0.001, 1))
    assert both.quantum_error("cx", (1, 0)) == two.expand(two).compose(depolarizing_error(0.01, 2))
    assert both.readout_flips(3) == (0.02, 0.02)
    with pytest.raises(ValueError):
        ibm_like_model(t1=100.0)
    with pytest.raises(ValueError):
        ibm_like_model(t1=100.0, t2=80.0, gate_time="35")
    with pytest.raises(ValueError):
        ibm_like_model(t1=10.0, t2=30.0, gate_time="35,300")
