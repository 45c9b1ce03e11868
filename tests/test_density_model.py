"""``run(method="density_matrix")`` on the host: the backend contract through a numpy stand-in engine, the mirror rule of
unitary records, the Pauli coefficient table of the library, and the ambiguity cap of the device sampling cases."""
import json

import numpy as np
import pytest

import _density_cases as dc
import _kraus_cases as kc
import _noise_exact_cases as nc
from _density_matrix import NoisyNumpyEngine, _gate_rows, _pauli_channel, _records
from _kraus_reference import KrausNumpyEngine, kraus_density_distribution
from qcmrf_amd import QCMRF, _lib, ingest as ing_mod, ir, program
from qcmrf_amd.backend import QsvBackend, _format_keys
from qcmrf_amd.comm import SingleProcess
from qcmrf_amd.transpile import transpile


@pytest.fixture()
def dbe():
    b = QsvBackend()
    b._engine_factory = dc.DensityNumpyEngine
    dc.DensityNumpyEngine.free_bytes = 1 << 40
    yield b
    b.close()


def lowered(j, rep=1):
    g = nc.models_05()
    return transpile(QCMRF(g["GRAPHS"][j], g["THETAS"][str(j)][rep], with_measurements=True), basis_gates=nc.BASIS)


def reference(qc, nm):
    """(distribution over the classical register as an array, Ingested)"""
    ing = ing_mod.ingest(qc, noise=nm)
    rec, data = program.encode(ing.ops)
    meas = [ing.measure.get(c, -1) for c in range(ing.num_clbits)]
    ro = [ing.readout.get(c, (0.0, 0.0)) for c in range(ing.num_clbits)] if ing.readout else None
    return kraus_density_distribution(rec, data, ing.num_qubits, meas, ro), ing


def as_array(probs, nbits):
    out = np.zeros(1 << nbits)
    for k, v in probs.items():
        out[int(k.replace(" ", ""), 2)] = v
    return out


# ---- the distribution through the whole host path ---------------------------------------------------------------------------

@pytest.mark.parametrize("j", [0, 1, 2, 5])
def test_probabilities_of_lowered_reference_graphs_under_the_thermal_model(dbe, j):
    T, nm = lowered(j), kc.thermal_model()
    want, ing = reference(T, nm)
    res = dbe.run(T, shots=0, method="density_matrix", noise_model=nm).result()
    probs = res.get_probabilities()
    got = as_array(probs, ing.num_clbits)
    print("DENSITY host graph %d: W=%d, %d records, max |p - reference| = %.3g" % (j, ing.num_qubits, res.metadata(0)["n_device_ops"],
                                                                                 np.abs(got - want).max()))
    assert np.abs(got - want).max() <= 1e-10
    assert all(v > 0 for v in probs.values()) and len(probs) == int((want > 0).sum())
    assert res.get_counts() == {}


# ---- backend contract -----------------------------------------------------------------------------------------------------------

def test_probabilities_sum_to_one_metadata_counts_and_seed(dbe):
    T, nm = lowered(1), kc.thermal_model()
    res = dbe.run(T, shots=3000, seed_simulator=11, method="density_matrix", noise_model=nm).result()
    probs, counts, meta = res.get_probabilities(), res.get_counts(), res.metadata(0)
    assert abs(sum(probs.values()) - 1.0) <= 1e-12
    assert sum(counts.values()) == 3000 and set(counts) <= set(probs)
    assert all(len(k) == T.num_clbits for k in probs)
    ing = ing_mod.ingest(T, noise=nm)
    assert meta["method"] == "density_matrix" and meta["n_qubits"] == 4 and meta["state_bytes"] == 16 * 4 ** 4
    assert meta["n_device_ops"] == len(program.encode(ing.ops)[0])
    assert meta["n_pauli_ops"] == ing.n_pauli > 0 and meta["n_kraus_ops"] == ing.n_kraus > 0
    assert abs(meta["trace"] - 1.0) <= 1e-12
    for k in ("time_compile", "time_evolve", "time_sample", "time_taken", "seed_simulator"):
        assert k in meta
    eng = dc.DensityNumpyEngine.made[-1]
    assert eng.n_qubits == 8 and eng.calls == ["density_exec", "density_diagonal", "density_sample"]
    again = dbe.run(T, shots=3000, seed_simulator=11, method="density_matrix", noise_model=nm).result().get_counts()
    other = dbe.run(T, shots=3000, seed_simulator=12, method="density_matrix", noise_model=nm).result().get_counts()
    assert again == counts and other != counts
    json.dumps(res.to_dict())


def test_shots_zero_gives_no_counts_but_the_distribution(dbe):
    res = dbe.run(lowered(0), shots=0, method="density_matrix", noise_model=kc.thermal_model()).result()
    assert res.get_counts() == {} and abs(sum(res.get_probabilities().values()) - 1.0) <= 1e-12
    assert "density_sample" not in dc.DensityNumpyEngine.made[-1].calls


@pytest.mark.parametrize("model", [None, "empty"])
def test_no_model_or_an_ideal_one_gives_the_ideal_distribution(dbe, model):
    from oracle import closed_form as cf
    from qcmrf_amd.noise import NoiseModel
    g = nc.models_05()
    C, th = g["GRAPHS"][1], g["THETAS"]["1"][2]
    qc = QCMRF(C, th, with_measurements=True)
    res = dbe.run([qc, lowered(1, 2)], shots=10, method="density_matrix", noise_model=NoiseModel() if model else None).result()
    want = cf.probabilities(C, th)
    for probs in res.get_probabilities():
        assert np.abs(as_array(probs, qc.num_clbits) - want).max() <= 1e-10
    assert res.metadata(0)["n_pauli_ops"] == 0 and res.metadata(1)["n_kraus_ops"] == 0


def test_get_probabilities_by_index_and_name_and_not_for_other_methods(dbe):
    a, b = lowered(0), lowered(1)
    res = dbe.run([a, b], shots=0, method="density_matrix").result()
    both = res.get_probabilities()
    assert isinstance(both, list) and len(both) == 2
    assert res.get_probabilities(1) == both[1] and res.get_probabilities(a) == both[0]
    k = QsvBackend()
    k._engine_factory = lambda n, devices=(0,), rank=None, world_size=None: KrausNumpyEngine(n, len(devices))
    plain = k.run(a, shots=10, noise_model=kc.thermal_model()).result()
    with pytest.raises(ValueError, match="density_matrix"):
        plain.get_probabilities()


def test_unwritten_classical_bits_stay_zero_in_the_keys(dbe):
    from qcmrf_amd.circuit import QuantumCircuit
    qc = QuantumCircuit(3, 4)
    qc.h(0)
    qc.cx(0, 2)
    qc.x(1)
    qc.measure(1, 0)
    qc.measure(2, 3)                                               # classical bits 1 and 2 are never written
    res = dbe.run(qc, shots=200, seed_simulator=3, method="density_matrix").result()
    probs = res.get_probabilities()
    assert set(probs) == {"0001", "1001"} and all(abs(v - 0.5) <= 1e-12 for v in probs.values())
    assert set(res.get_counts()) <= set(probs) and sum(res.get_counts().values()) == 200


class _Group(SingleProcess):
    world = 2


def test_refusals_name_their_limits(dbe):
    from qcmrf_amd.circuit import QuantumCircuit
    wide = QuantumCircuit(_lib.DENSITY_MAX_QUBITS + 1, 1)
    wide.h(0)
    wide.measure(0, 0)
    with pytest.raises(ValueError, match="at most %d qubits" % _lib.DENSITY_MAX_QUBITS):
        dbe.run(wide, shots=1, method="density_matrix")
    many = QuantumCircuit(2, 21)
    many.h(0)
    for c in range(21):
        many.measure(c % 2, c)
    with pytest.raises(ValueError, match="at most 20 written classical bits"):
        dbe.run(many, shots=1, method="density_matrix")
    dc.DensityNumpyEngine.free_bytes = 16 * 4 ** 4 - 1
    with pytest.raises(ValueError, match="%d bytes.*%d free" % (16 * 4 ** 4, 16 * 4 ** 4 - 1)):
        dbe.run(lowered(1), shots=1, method="density_matrix")
    dc.DensityNumpyEngine.free_bytes = 16 * 4 ** 4
    dbe.run(lowered(1), shots=1, method="density_matrix")
    with pytest.raises(ValueError, match="2 ranks.*limit 1"):
        dbe.run(lowered(0), shots=1, method="density_matrix", comm=_Group())
    with pytest.raises(TypeError):
        dbe.run(lowered(0), shots=1, method="density_matrix", noise_model="depolarizing")


def test_unknown_method_is_refused():
    b = QsvBackend()
    b._engine_factory = dc.DensityNumpyEngine
    with pytest.raises(ValueError, match="unknown method 'matrix_product_state'.*density_matrix"):
        b.run(lowered(0), shots=1, method="matrix_product_state")
    with pytest.raises(ValueError, match="unknown method"):
        QsvBackend(method="densitymatrix").run(lowered(0), shots=1)


def test_a_noisy_run_without_method_still_takes_the_trajectory_kernel():
    b = QsvBackend()
    b._engine_factory = lambda n, devices=(0,), rank=None, world_size=None: KrausNumpyEngine(n, len(devices))
    before = NoisyNumpyEngine.calls
    res = b.run(lowered(1), shots=50, seed_simulator=1, noise_model=kc.thermal_model()).result()
    assert NoisyNumpyEngine.calls == before + 1 and res.metadata(0)["method"] == "noisy"
    res = b.run(lowered(1), shots=50, seed_simulator=1, noise_model=kc.thermal_model(), method="statevector").result()
    assert NoisyNumpyEngine.calls == before + 2 and res.metadata(0)["method"] == "noisy"


def test_run_experiment_writes_the_distributions(tmp_path, monkeypatch):
    from qcmrf_amd import backend as be_mod, run_experiment
    b = QsvBackend()
    b._engine_factory = dc.DensityNumpyEngine
    monkeypatch.setattr(be_mod.Aer, "get_backend", lambda name="qasm_simulator", **o: b)
    import qcmrf_amd.workloads as wl
    monkeypatch.setattr(wl, "REFERENCE_GRAPHS", wl.REFERENCE_GRAPHS[:2])
    counts = run_experiment.main(["--scale", "0.5", "--shots", "100", "--reps", "1", "--outdir", str(tmp_path), "--seed-simulator", "5",
                                  "--method", "density_matrix", "--depolarizing", "0.001,0.01", "--readout", "0.02"])
    probs = json.load(open(tmp_path / "probs_simulation_noisy_0.5.json"))
    saved = json.load(open(tmp_path / "result_simulation_noisy_0.5.json"))
    assert saved == counts and len(probs) == len(counts) == 2
    for p, c in zip(probs, counts):
        assert abs(sum(p.values()) - 1.0) <= 1e-12 and set(c) <= set(p) and sum(c.values()) == 100


# ---- the mirror rule, independent of any engine ----------------------------------------------------------------------------------

def mirror(rec, data, W):
    """the records of a unitary program on the ket bits, each followed by its mirror on the bra bits (include/qsv.h):
    qubits + W, matrix and table conjugated, angle negated, MCX as it is"""
    data = np.array(data, dtype=np.float64)
    out = []
    for r in rec:
        bra = r.copy()
        n = int(r["n"])
        bra["target"] = r["target"] + W
        bra["qubits"][:n] = r["qubits"][:n] + W
        bra["angle"] = -r["angle"]
        kind = int(r["kind"])
        cnt = 8 if kind == _lib.OP_1Q else ((2 << n) if kind == _lib.OP_DIAG else 0)
        if cnt:
            conj = data[int(r["data_off"]):int(r["data_off"]) + cnt].copy()
            conj[1::2] *= -1.0
            bra["data_off"] = data.size
            data = np.concatenate([data, conj])
        out += [r, bra]
    return np.array(out, dtype=rec.dtype), data


@pytest.mark.parametrize("kind", ["u", "x", "diag", "mcphase"])
def test_mirrored_pair_on_vec_rho_is_u_rho_udg(kind):
    W = 4
    rng = np.random.RandomState({"u": 1, "x": 2, "diag": 3, "mcphase": 4}[kind])
    a = rng.randn(1 << W, 1 << W) + 1j * rng.randn(1 << W, 1 << W)
    rho = a @ a.conj().T
    rho /= np.trace(rho).real
    U = nc._unitary(rng)
    for ctrls, vals in (([], []), ([3], [1]), ([0, 2], [0, 1]), ([2, 3, 0], [1, 0, 0])):
        op = {"u": lambda: ir.op_u(1, U, ctrls, vals), "x": lambda: ir.op_x(1, ctrls, vals),
              "diag": lambda: ir.op_diag([1] + ctrls, np.exp(2j * np.pi * rng.rand(2 << len(ctrls)))),
              "mcphase": lambda: ir.op_mcphase([1] + ctrls, 0.37 + len(ctrls), [1] + vals)}[kind]()
        rec, data = program.encode([op])
        (k, t, qs, vs, off, mask, angle), = _records(rec, np.asarray(data))
        full = _gate_rows(np.eye(1 << W, dtype=np.complex128), k, t, qs, vs, off, mask, angle, np.asarray(data, dtype=np.float64))
        want = full @ rho @ full.conj().T
        mrec, mdata = mirror(rec, data, W)
        vec = dc.vec_of(rho).reshape(-1, 1).copy()
        for k, t, qs, vs, off, mask, angle in _records(mrec, mdata):
            vec = _gate_rows(vec, k, t, qs, vs, off, mask, angle, mdata)
        assert np.abs(vec.ravel() - dc.vec_of(want)).max() <= 1e-14
        assert np.abs(want - rho).max() > 1e-3                    # the record did something


def test_mirrored_init_uniform_is_the_outer_product():
    from _density_matrix import _init_vector
    W, m = 3, 0b101
    v = _init_vector(1 << W, _lib.OP_INIT_UNIFORM, m)
    both = _init_vector(1 << (2 * W), _lib.OP_INIT_UNIFORM, m | (m << W))
    assert np.abs(both - dc.vec_of(np.outer(v, v.conj()))).max() <= 1e-16


# ---- the Pauli coefficient table of the library (host code of qsv_density_exec) ---------------------------------------------------

def apply_table(rho, qs, c):
    """out[v] = sum_x c[x, d(v)] in[v ^ m_x] on rho[i, j] directly"""
    N = rho.shape[0]
    i, j = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    d = np.zeros_like(i)
    for b, q in enumerate(qs):
        d |= (((i ^ j) >> q) & 1) << b
    out = np.zeros_like(rho)
    for x in range(1 << len(qs)):
        m = sum(((x >> b) & 1) << q for b, q in enumerate(qs))
        out += c[x][d] * rho[i ^ m, j ^ m]
    return out


def _random_rho(rng, W):
    a = rng.randn(1 << W, 1 << W) + 1j * rng.randn(1 << W, 1 << W)
    rho = a @ a.conj().T
    return rho / np.trace(rho).real


def test_pauli_table_reproduces_the_channel_for_every_single_pauli_and_random_tables():
    rng = np.random.RandomState(5)
    W = 3
    rho = _random_rho(rng, W)
    cases = [((1,), np.eye(4)[p]) for p in range(1, 4)] + [(qs, np.eye(16)[p]) for qs in ((0, 2), (2, 1)) for p in range(1, 16)]
    cases += [((q,), rng.dirichlet(np.ones(4))) for q in range(W)] + [(qs, rng.dirichlet(np.ones(16))) for qs in ((0, 1), (2, 0), (1, 2))]
    for qs, probs in cases:
        cum = np.cumsum(probs)
        cum[-1] = 1.0
        c = _lib.density_pauli_table(len(qs), cum)
        got = apply_table(rho, qs, c)
        want = _pauli_channel(rho, list(qs), np.diff(np.concatenate([[0.0], cum])))
        assert np.abs(got - want).max() <= 1e-15, (qs, probs)
    with pytest.raises(ValueError):
        _lib.density_pauli_table(3, np.ones(64))


# ---- the ambiguity cap of the device sampling cases, on the reference alone -----------------------------------------------------------

@pytest.mark.parametrize("name", list(dc.SAMPLE_CASES))
def test_reference_of_every_sampling_case_is_within_the_cap(name):
    words, alt, amb, diag = dc.sample_reference(name)
    cap = nc.ambiguity_cap(words.size)
    print("DENSITY reference case=%s shots=%d ambiguous=%d cap=%d" % (name, words.size, int(amb.sum()), cap))
    assert int(amb.sum()) <= cap
    assert abs(diag.sum() - 1.0) <= 1e-12
    nc.check_words(words.copy(), words, alt, amb, family="density self", label=name)


def test_stand_in_sampling_follows_its_distribution():
    from _density_matrix import chi2_pvalue, word_distribution
    c = dc.sample_case("seed 0x0")
    words, _, _, diag = dc.sample_reference("seed 0x0")
    want = word_distribution(np.clip(diag, 0, None), c["meas"], c["readout"])
    uv, uc = np.unique(words, return_counts=True)
    assert chi2_pvalue(_format_keys(uv, uc, len(c["meas"]), None), want, words.size) > 1e-4
