"""Two-qubit Kraus channels on the host: the model (qcmrf_amd.noise), the encoded record (program.encode), ingest and the
in-place remapping."""
import numpy as np
import pytest

import _kraus2_cases as k2c
from qcmrf_amd import QCMRF, _lib, ingest as ing_mod, ir, program
from qcmrf_amd.backend import QsvBackend
from qcmrf_amd.noise import (NoiseModel, amplitude_damping_error, coherent_unitary_error, depolarizing_error, kraus_error,
                             mixed_unitary_error, pauli_error, thermal_relaxation_error, two_qubit_kraus_error)
from qcmrf_amd.run_experiment import cx_over_rotation, ibm_like_model

I2 = np.eye(2, dtype=np.complex128)
X = np.array([[0, 1], [1, 0]], dtype=np.complex128)
Z = np.diag([1.0 + 0j, -1.0])


def superop(ks):
    return sum(np.kron(k.conj(), k) for k in ks)


# ---- constructors -----------------------------------------------------------------------------------------------------------

def test_two_qubit_kraus_error_keeps_operators_and_refuses_non_channels():
    rng = np.random.RandomState(1)
    ks = k2c.isometry_kraus2(rng, 3)
    e = two_qubit_kraus_error(ks)
    assert e.num_qubits == 2 and not e.is_ideal() and not e.is_pauli()
    (kind, qs, stack), = e.terms()
    assert kind == "kraus2" and qs == (0, 1) and stack.shape == (3, 4, 4) and np.array_equal(stack, ks)
    assert np.abs(e.superoperator() - superop(ks)).max() < 1e-14
    with pytest.raises(ValueError, match="at least one"):
        two_qubit_kraus_error([])
    with pytest.raises(ValueError, match="4 x 4"):
        two_qubit_kraus_error([I2])
    with pytest.raises(ValueError, match="not a channel"):
        two_qubit_kraus_error([0.9 * np.eye(4)])
    with pytest.raises(ValueError, match="finite"):
        two_qubit_kraus_error([np.full((4, 4), np.nan)])
    with pytest.raises(ValueError, match="two-qubit Kraus"):
        kraus_error([np.eye(4)])                                      # the one-qubit constructor still refuses, and says where to go
    with pytest.raises(ValueError, match="one-qubit"):
        e.kraus()
    assert two_qubit_kraus_error([np.eye(4)]).is_ideal()
    with pytest.raises(ValueError):
        e.probabilities


def test_more_than_16_operators_become_the_canonical_set():
    rng = np.random.RandomState(2)
    ks = k2c.isometry_kraus2(rng, 20)
    e = two_qubit_kraus_error(ks)
    (_, _, stack), = e.terms()
    assert stack.shape == (16, 4, 4)
    assert np.abs(superop(stack) - superop(ks)).max() < 1e-14
    weights = [np.real(np.trace(k.conj().T @ k)) for k in stack]
    assert all(a >= b - 1e-15 for a, b in zip(weights, weights[1:]))               # Choi eigenvalues, descending
    low = two_qubit_kraus_error(list(k2c.correlated_damping(0.3)) + [np.zeros((4, 4))] * 16)
    assert low.terms()[0][2].shape == (2, 4, 4)                                   # eigenvalues below 1e-14 dropped


def test_product_given_as_4x4_operators_equals_the_product_form():
    t = thermal_relaxation_error(20e3, 30e3, 1500.0)
    prod = t.expand(t)
    dense = two_qubit_kraus_error([np.kron(b, a) for a in t.kraus() for b in t.kraus()])
    assert dense == prod and prod == dense
    assert [kind for kind, _, _ in prod.terms()] == ["kraus", "kraus"]            # tensor / expand keep the product form
    assert [kind for kind, _, _ in dense.terms()] == ["kraus2"]
    assert dense != t.expand(amplitude_damping_error(0.1))


def test_coherent_unitary_error():
    u2 = np.array([[np.cos(0.1), -1j * np.sin(0.1)], [-1j * np.sin(0.1), np.cos(0.1)]])
    assert coherent_unitary_error(u2) == kraus_error([u2])
    assert coherent_unitary_error(u2).terms()[0][0] == "kraus"
    u4 = cx_over_rotation(0.05)
    e = coherent_unitary_error(u4)
    (kind, _, stack), = e.terms()
    assert kind == "kraus2" and stack.shape == (1, 4, 4) and np.array_equal(stack[0], u4)
    with pytest.raises(ValueError, match="not unitary"):
        coherent_unitary_error(1.001 * u4)
    with pytest.raises(ValueError, match="2 x 2 or 4 x 4"):
        coherent_unitary_error(np.eye(3))


def test_mixed_unitary_error():
    rng = np.random.RandomState(3)
    u, v = k2c.unitary4(rng), k2c.unitary4(rng)
    e = mixed_unitary_error([(np.eye(4), 0.5), (u, 0.0), (v, 0.5)])
    (kind, _, stack), = e.terms()
    assert kind == "kraus2" and stack.shape == (2, 4, 4)                           # the p = 0 term is dropped
    assert np.abs(stack[1] - np.sqrt(0.5) * v).max() < 1e-15
    one = mixed_unitary_error([(I2, 0.9), (np.array([[1, 1], [1, -1]]) / np.sqrt(2.0), 0.1)])
    assert one.num_qubits == 1 and one.terms()[0][0] == "kraus"
    many = mixed_unitary_error([(k2c.unitary4(rng), 1.0 / 20)] * 20)
    assert many.terms()[0][2].shape[0] <= 16
    for bad in ([(u, 0.5), (v, 0.4)], [(u, -0.1), (v, 1.1)], [], [(u, 0.5), (I2, 0.5)], [(2 * u, 1.0)]):
        with pytest.raises(ValueError):
            mixed_unitary_error(bad)


def test_mixed_unitary_of_paulis_is_the_pauli_error():
    zx = np.kron(X, Z)                                                # Z on error qubit 0, X on error qubit 1
    e = mixed_unitary_error([(np.eye(4), 0.9), (zx, 0.07), (1j * np.kron(I2, X), 0.03)])
    want = pauli_error([("II", 0.9), ("XZ", 0.07), ("IX", 0.03)])
    assert e.is_pauli() and e == want and np.allclose(e.probabilities, want.probabilities, atol=1e-15)
    assert [kind for kind, _, _ in e.terms()] == ["pauli"]
    assert e.to_dict() == want.to_dict()
    assert mixed_unitary_error([(I2, 0.8), (X, 0.2)]) == pauli_error([("I", 0.8), ("X", 0.2)])
    # a dense set that is a Pauli channel comes out of a composition as a "pauli" op too
    dense = two_qubit_kraus_error([np.sqrt(0.9) * np.eye(4), np.sqrt(0.1) * zx])
    both = dense.compose(pauli_error([("II", 1.0)]))
    assert [kind for kind, _, _ in both.terms()] == ["pauli"]


# ---- algebra ----------------------------------------------------------------------------------------------------------------

def test_compose_and_merge_multiply_the_superoperators():
    rng = np.random.RandomState(4)
    a, b = two_qubit_kraus_error(k2c.isometry_kraus2(rng, 2)), coherent_unitary_error(cx_over_rotation(0.3))
    t = thermal_relaxation_error(20e3, 30e3, 1500.0)
    prod, dep = t.expand(t), depolarizing_error(0.05, 2)
    for first, second in ((a, b), (b, a), (prod, b), (b, prod), (dep, a), (a, dep)):
        c = first.compose(second)
        assert np.abs(c.superoperator() - second.superoperator() @ first.superoperator()).max() < 1e-13
        assert [kind for kind, _, _ in c.terms()] == ["kraus2"]                   # one record, not several
    three = prod.compose(dep).compose(b)
    assert [kind for kind, _, _ in three.terms()] == ["kraus2"] and three.terms()[0][2].shape[0] <= 16
    assert np.abs(three.superoperator() - b.superoperator() @ dep.superoperator() @ prod.superoperator()).max() < 1e-13
    assert [kind for kind, _, _ in prod.compose(dep).terms()] == ["kraus", "kraus", "pauli"]      # as before
    with pytest.raises(ValueError):
        a.compose(t)
    with pytest.raises(ValueError):
        a.tensor(t)


def test_noise_model_accepts_the_new_errors():
    b = coherent_unitary_error(cx_over_rotation(0.3))
    nm = NoiseModel()
    nm.add_all_qubit_quantum_error(depolarizing_error(0.01, 2), ["cx"])
    nm.add_all_qubit_quantum_error(b, ["cx"])
    nm.add_quantum_error(b, ["cx"], [2, 0])
    assert nm.quantum_error("cx", (0, 1)) == depolarizing_error(0.01, 2).compose(b)
    assert nm.quantum_error("cx", (2, 0)) == b
    with pytest.raises(ValueError, match="2-qubit error"):
        nm.add_all_qubit_quantum_error(b, ["sx"])
        nm.quantum_error("sx", (0,))
    only = ibm_like_model(coherent_cx=0.05)
    assert only.quantum_error("cx", (0, 1)) == coherent_unitary_error(cx_over_rotation(0.05)) and only.quantum_error("sx", (0,)) is None
    both = ibm_like_model(depolarizing="0.001,0.01", coherent_cx=0.05)
    assert both.quantum_error("cx", (0, 1)) == depolarizing_error(0.01, 2).compose(coherent_unitary_error(cx_over_rotation(0.05)))
    assert ibm_like_model() is None


# ---- qubit order, record layout, ingest ---------------------------------------------------------------------------------------

def test_error_qubit_0_is_the_gates_first_argument():
    """a 4 x 4 I (x) K acts on error qubit 0 only; behind cx(2, 0) that is qubit 2"""
    damp = amplitude_damping_error(1.0).kraus()
    e = two_qubit_kraus_error([np.kron(I2, k) for k in damp])
    assert e == amplitude_damping_error(1.0).expand(kraus_error([I2]))           # other (x) self: self on error qubit 0
    nm = NoiseModel()
    nm.add_all_qubit_quantum_error(e, ["cx"])
    from qcmrf_amd.circuit import QuantumCircuit
    qc = QuantumCircuit(3, 3)
    qc.x(0)
    qc.x(2)
    qc.cx(2, 0)                                                       # |101> -> |100>; the error then empties qubit 2
    qc.measure([0, 1, 2], [0, 1, 2])
    ing = ing_mod.ingest(qc, noise=nm)
    k2 = [op for op in ing.ops if op.kind == "kraus2"]
    assert len(k2) == 1 and k2[0].qubits == (2, 0) and ing.n_kraus2 == 1 and ing.n_kraus == 0 and ing.n_pauli == 0
    assert [op.kind for op in ing.ops][-2:] == ["x", "kraus2"]                     # behind its gate
    rec, data = program.encode(ing.ops)
    dist = k2c.kraus2_density_distribution(rec, data, 3, [0, 1, 2])
    assert abs(dist[0b000] - 1.0) < 1e-14                             # qubit 2 (the first argument) was damped, qubit 0 was 0 already
    nm2 = NoiseModel()
    nm2.add_all_qubit_quantum_error(two_qubit_kraus_error([np.kron(k, I2) for k in damp]), ["cx"])       # error qubit 1 = qubit 0
    rec, data = program.encode(ing_mod.ingest(qc, noise=nm2).ops)
    assert abs(k2c.kraus2_density_distribution(rec, data, 3, [0, 1, 2])[0b100] - 1.0) < 1e-14


def test_encode_lays_the_record_out_as_documented():
    rng = np.random.RandomState(5)
    ks = k2c.isometry_kraus2(rng, 3)
    op = k2c.kraus2_op(4, 1, ks)
    rec, data = program.encode([op, k2c.kraus2_op(0, 2, ks)])
    r = rec[0]
    assert r["kind"] == _lib.OP_KRAUS2 == 12 and r["n"] == 2 and list(r["qubits"][:2]) == [4, 1] and r["vals"][0] == 3
    off = int(r["data_off"])
    K = data[off:off + 96].view(np.complex128).reshape(3, 4, 4)
    assert np.array_equal(K, ks)                                      # row-major, (re, im)
    E = data[off + 96:off + 144].reshape(3, 16)
    for k in range(3):
        full = ks[k].conj().T @ ks[k]
        assert np.allclose(E[k, :4], np.real(np.diag(full)), atol=1e-16)
        for j, (a, b) in enumerate(((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))):
            assert abs(complex(E[k, 4 + 2 * j], E[k, 5 + 2 * j]) - full[a, b]) < 1e-16
    assert np.array_equal(program.kraus2_tables(ks), data[off:off + 144])
    with pytest.raises(ValueError, match="1 to 16"):
        program.kraus2_tables(k2c.isometry_kraus2(rng, 17))
    with pytest.raises(ValueError, match="sum K"):
        program.kraus2_tables(0.5 * ks)
    with pytest.raises(ValueError, match="distinct"):
        program.encode([k2c.kraus2_op(1, 1, ks)])
    assert ir.Op("kraus2", qubits=(4, 1), table=ks).support() == (4, 1)


def test_in_place_measurement_remaps_the_two_qubits_like_a_pauli_op():
    """the same circuit under a two-qubit Pauli error and under a dense error on cx: in place, the kraus2 ops sit where the
    pauli ops sit, on the same (remapped) qubit pairs in the same order"""
    T = k2c.chain3(True)
    models = []
    for e in (depolarizing_error(0.02, 2), coherent_unitary_error(cx_over_rotation(0.2))):
        nm = NoiseModel()
        nm.add_all_qubit_quantum_error(e, ["cx"])
        models.append(nm)
    streams = []
    for nm in models:
        ing, rec, data, clist, meas, readout, _, state, (mode, width, n_measure) = QsvBackend._prepare_noisy(T, nm, "lds", "in_place")
        assert mode == "in_place" and width == 5 and n_measure > 0
        streams.append(ing.ops)
    pauli, dense = streams
    assert len(pauli) == len(dense)
    assert [o.kind for o in dense] == [{"pauli": "kraus2"}.get(o.kind, o.kind) for o in pauli]
    assert [o.qubits for o in dense if o.kind == "kraus2"] == [o.qubits for o in pauli if o.kind == "pauli"]
    deferred = [o.qubits for o in ing_mod.ingest(T, noise=models[1]).ops if o.kind == "kraus2"]
    assert deferred != [o.qubits for o in dense if o.kind == "kraus2"] and max(max(q) for q in deferred) == 5
    assert max(max(o.qubits) for o in dense if o.kind == "kraus2") <= 4
