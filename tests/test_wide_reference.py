"""Host checks of the wide noisy-shot reference (_wide_reference.py) and of the backend's ``noisy_state`` option: the
reference agrees bit for bit with the narrow one where both work, every wide device case is free of boundary
ambiguity by the reference alone, the word comparison notices the mistakes a wide kernel could make, and the backend
refuses what it must before any device is needed."""
import numpy as np
import pytest

import _kraus_cases as kc
import _noise_exact_cases as nc
import _wide_reference as wr
from _kraus_reference import check_kraus_words, exact_kraus_sample, within_cap
from qcmrf_amd import _lib, program
from qcmrf_amd.backend import QsvBackend
from qcmrf_amd.circuit import QuantumCircuit
from qcmrf_amd.noise import NoiseModel, ReadoutError, amplitude_damping_error, depolarizing_error


@pytest.mark.parametrize("W", [3, 7, 11])
def test_wide_reference_is_the_narrow_reference_up_to_13_qubits(W):
    ops = kc.with_kraus(nc.random_ops(W, 9000 + W, n_random=32, init=nc.WIDTH_INIT[W]), W, np.random.RandomState(9500 + W))
    rec, data = program.encode(ops)
    meas = [W - 1, -1, 0] + list(range(W))
    ro = np.random.RandomState(W).uniform(0.0, 0.2, (len(meas), 2))
    shots = 64 if W > 7 else 300
    for tail in ((None, None), (meas, ro)):
        narrow = exact_kraus_sample(rec, data, W, shots, 9900 + W, *tail)
        wide = wr.exact_wide_sample(rec, data, W, shots, 9900 + W, *tail)
        for a, b in zip(narrow, wide):
            assert a.dtype == b.dtype and np.array_equal(a, b)
    part = wr.exact_wide_sample(rec, data, W, 20, 9900 + W, first_shot=17)
    assert np.array_equal(part[0], wr.exact_wide_sample(rec, data, W, 64, 9900 + W)[0][17:37])


def test_parity_is_a_popcount():
    v = np.array([0, 1, 3, 7, 2 ** 13, 2 ** 16 | 1, 2 ** 23 | 2 ** 16 | 2 ** 3, 2 ** 24 - 1])
    assert wr.parity(v).tolist() == [bin(int(x)).count("1") & 1 for x in v]


@pytest.mark.parametrize("name", list(wr.WIDE_CASES))
def test_wide_cases_have_no_ambiguous_shot(name):
    words, alt, amb, undet = wr.reference(name)
    c = wr.case(name)
    assert words.size == c["shots"]
    n, cap = within_cap(amb, undet)
    assert cap == 2 and n == 0
    assert np.array_equal(words, alt)
    if c["meas"] is None:
        assert int(words.max()) >> (c["W"] - 1) == 1            # the top qubit is populated: the words need all W bits
    else:
        assert (words < 2 ** len(c["meas"])).all()


def test_wide_case_17_uses_qubit_16_everywhere_a_record_can():
    rec = wr.case("W=17")["rec"]
    listed = lambda k: {int(q) for r in rec[rec["kind"] == k] for q in r["qubits"][:r["n"]]}
    assert 16 in listed(_lib.OP_PAULI) and 16 in listed(_lib.OP_DIAG) and 16 in listed(_lib.OP_KRAUS)
    assert 16 in listed(_lib.OP_1Q) | listed(_lib.OP_MCX)          # a control on qubit 16: mask bit 16
    assert 16 in {int(t) for t in rec[(rec["kind"] == _lib.OP_1Q) | (rec["kind"] == _lib.OP_MCX)]["target"]}


@pytest.mark.parametrize("how", wr.MUTATIONS)
def test_comparison_notices_a_wrong_wide_kernel(how):
    c = wr.case("W=17")
    good = wr.reference("W=17")
    check_kraus_words(good[0], *good, family="wide host", label="the reference against itself")
    bad = wr.reference_of(c, _mutate=how)[0]
    with pytest.raises(AssertionError, match="differ"):
        check_kraus_words(bad, *good, family="wide host", label=how)
    with pytest.raises(ValueError):
        wr.reference_of(c, _mutate="nothing")


# ---- the backend's noisy_state option ---------------------------------------------------------------------------------------

def model():
    nm = NoiseModel()
    nm.add_all_qubit_quantum_error(depolarizing_error(0.02, 1), ["h", "x"])
    nm.add_all_qubit_quantum_error(amplitude_damping_error(0.05), ["id"])
    nm.add_all_qubit_readout_error(ReadoutError([[0.97, 0.03], [0.05, 0.95]]))
    return nm


def top_qubit_circuit(n, clbits=1, bit=0):
    qc = QuantumCircuit(n, clbits)
    qc.x(n - 1)
    qc.measure(n - 1, bit)
    return qc


class RecordingEngine:
    """stands in for libqsv: says which entry point a run took"""
    calls = []

    def __init__(self, n_qubits, devices=(0,), rank=None, world_size=None):
        self.n_qubits = n_qubits

    def set_option(self, name, value):
        pass

    def noisy_sample(self, ops, data, shots, seed, meas_qubits=None, readout=None):
        RecordingEngine.calls.append(("lds", self.n_qubits))
        return np.zeros(shots, dtype=np.uint64)

    def noisy_sample_hbm(self, ops, data, shots, seed, meas_qubits=None, readout=None):
        RecordingEngine.calls.append(("hbm", self.n_qubits))
        return np.ones(shots, dtype=np.uint64)

    def close(self):
        pass


@pytest.fixture
def rbe():
    b = QsvBackend()
    b._engine_factory = RecordingEngine
    RecordingEngine.calls = []
    yield b
    b.close()


def test_constants_and_binding():
    assert _lib.NOISY_MAX_QUBITS == 13 and _lib.NOISY_HBM_MAX_QUBITS == 24
    assert _lib.SIGNATURES["qsv_noisy_sample_hbm"] == _lib.SIGNATURES["qsv_noisy_sample"]
    assert callable(_lib.Engine.noisy_sample_hbm)
    assert QsvBackend().options["noisy_state"] == "lds"


def test_noisy_state_routes_to_the_entry_point(rbe):
    nm = model()
    for state, n, want in (("lds", 5, "lds"), ("auto", 5, "lds"), ("auto", 13, "lds"), ("auto", 14, "hbm"), ("hbm", 5, "hbm"),
                           ("hbm", 14, "hbm"), ("hbm", 24, "hbm"), ("auto", 24, "hbm")):
        res = rbe.run(top_qubit_circuit(n), shots=20, seed_simulator=1, noise_model=nm, noisy_state=state).result()
        assert RecordingEngine.calls[-1] == (want, n)
        assert res.metadata(0)["method"] == "noisy" and res.metadata(0)["noisy_state"] == want
        assert res.get_counts() == {"1" if want == "hbm" else "0": 20}
    res = rbe.run(top_qubit_circuit(5), shots=20, seed_simulator=1, noise_model=nm).result()          # the default
    assert RecordingEngine.calls[-1] == ("lds", 5) and res.metadata(0)["noisy_state"] == "lds"
    rbe.set_options(noisy_state="hbm")
    rbe.run(top_qubit_circuit(5), shots=20, seed_simulator=1, noise_model=nm)
    assert RecordingEngine.calls[-1] == ("hbm", 5)


def test_noisy_state_refusals_need_no_device():
    be = QsvBackend()                                             # no engine factory: an engine would need a GPU
    nm = model()
    for bad in ("HBM", "global", "", None, 1):
        with pytest.raises(ValueError, match="noisy_state"):
            be.run(top_qubit_circuit(3), shots=10, noise_model=nm, noisy_state=bad)
    with pytest.raises(ValueError, match="13"):
        be.run(top_qubit_circuit(14), shots=10, noise_model=nm, noisy_state="lds")
    with pytest.raises(ValueError, match="13"):
        be.run(top_qubit_circuit(14), shots=10, noise_model=nm)
    for state in ("hbm", "auto"):
        with pytest.raises(ValueError, match="24"):
            be.run(top_qubit_circuit(25), shots=10, noise_model=nm, noisy_state=state)
        with pytest.raises(ValueError, match="64"):
            be.run(top_qubit_circuit(14, 65, 64), shots=10, noise_model=nm, noisy_state=state)
        with pytest.raises(ValueError, match="trajectory"):
            be.run(top_qubit_circuit(14), shots=10, noise_model=nm, noisy_state=state, method="trajectory")

        class TwoRanks:
            world, rank = 2, 0
        with pytest.raises(ValueError, match="limit 1"):
            be.run(top_qubit_circuit(14), shots=10, noise_model=nm, noisy_state=state, comm=TwoRanks())
    assert be._engine is None
