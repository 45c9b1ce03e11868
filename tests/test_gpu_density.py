"""The density-matrix method on the MI355X: ``qsv_density_exec`` / ``_diagonal`` / ``_sample`` against the numpy rho of
``_density_cases`` (amplitudes within 1e-12, probabilities within 1e-10: the project's two promises), sampling word by word
against the Philox contract, and ``run(method="density_matrix")`` end to end.

Word-by-word comparisons go through ``check_words``: a draw within 1e-9 of the total of a cumulative boundary may land on
the neighbour, at most max(2, shots // 1000) such shots per case (test_density_model.py asserts on the host that the
reference of every case stays within that cap on its own)."""
import numpy as np
import pytest

import _density_cases as dc
import _kraus_cases as kc
import _noise_exact_cases as nc
from _density_matrix import chi2_pvalue
from _kraus_reference import kraus_density_distribution
from qcmrf_amd import QCMRF, _lib, ingest as ing_mod, ir, program
from qcmrf_amd.backend import QsvBackend
from qcmrf_amd.transpile import transpile

pytestmark = pytest.mark.gpu

AMP_TOL, PROB_TOL = 1e-12, 1e-10


def check_state(eng, rho, W, label):
    """whole vector, Hermiticity, trace; the diagonal over all qubits, subsets and permuted subsets"""
    got = eng.amplitudes()
    err = float(np.abs(got - dc.vec_of(rho)).max())
    G = got.reshape(1 << W, 1 << W).T                               # G[i, j] = rho[i, j]
    herm = float(np.abs(G - G.conj().T).max())
    full, trace = eng.density_diagonal(list(range(W)))
    print("DENSITY %s: W=%d max |amp - reference| = %.3g, Hermiticity %.3g, |trace - 1| = %.3g" % (label, W, err, herm, abs(trace - 1.0)))
    assert err <= AMP_TOL
    assert herm <= AMP_TOL
    assert abs(trace - 1.0) <= AMP_TOL
    diag = np.real(np.diag(rho))
    assert np.abs(full - diag).max() <= PROB_TOL
    rng = np.random.RandomState(W)
    subsets = [[0], [W - 1], list(range(W))[::-1], [int(q) for q in rng.permutation(W)[:max(1, W // 2)]],
               [int(q) for q in rng.permutation(W)[:max(1, W - 1)]], []]
    for qs in subsets:
        m, tr = eng.density_diagonal(qs)
        assert m.shape == (1 << len(qs),) and tr == trace            # the same bits every time
        assert np.abs(m - dc.marginal(diag, qs)).max() <= PROB_TOL, qs


# ---- record level ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W", dc.WIDTHS)
def test_random_program_whole_vector(W):
    rec, data, rho = dc.width_case(W)
    kinds = set(int(k) for k in rec["kind"])
    want = {_lib.OP_1Q, _lib.OP_MCX, _lib.OP_DIAG, _lib.OP_MCPHASE, _lib.OP_PAULI, _lib.OP_KRAUS}
    assert want <= kinds
    kr = rec[rec["kind"] == _lib.OP_KRAUS]
    assert set(int(m) for m in kr["vals"][:, 0]) == {1, 2, 3, 4}
    assert set(int(q) for q in kr["qubits"][:, 0]) == {q for q in (0, 5, W - 1) if q < W}
    if W >= 4:
        pairs = {(int(a), int(b)) for a, b in rec[(rec["kind"] == _lib.OP_PAULI) & (rec["n"] == 2)]["qubits"][:, :2]}
        assert (0, W - 1) in pairs and (W - 1, 0) in pairs
    with _lib.Engine(2 * W) as eng:
        eng.density_exec(rec, data)
        check_state(eng, rho, W, "random program")
        eng.density_exec(rec, data)                                  # a second program starts from |0..0><0..0| again
        assert float(np.abs(eng.amplitudes() - dc.vec_of(rho)).max()) <= AMP_TOL


def test_w11_bra_bit_of_qubit_0_on_address_bit_11():
    rec, data, rho = dc.w11_case()
    assert len(rec) <= 12
    with _lib.Engine(22) as eng:
        eng.density_exec(rec, data)
        check_state(eng, rho, 11, "W=11")


@pytest.mark.parametrize("W", [2, 7])
def test_adjacent_and_distant_pauli_pairs_in_both_orders(W):
    """every two-qubit PAULI placement on its own, on a generic state"""
    rng = np.random.RandomState(70 + W)
    pairs = sorted({(0, 1), (1, 0), (0, W - 1), (W - 1, 0), (W - 2, W - 1), (W - 1, W - 2), (1, W - 2) if W > 3 else (0, 1), (5, 0) if W > 5 else (1, 0)})
    with _lib.Engine(2 * W) as eng:
        for qs in pairs:
            ops = [ir.op_u(q, nc._unitary(rng)) for q in range(W)] + [ir.op_x(qs[0], [qs[1]], [1]), nc._pauli(rng, list(qs))]
            rec, data = program.encode(ops)
            eng.density_exec(rec, data)
            err = float(np.abs(eng.amplitudes() - dc.vec_of(dc.numpy_rho(rec, data, W))).max())
            assert err <= AMP_TOL, (qs, err)


# ---- forced channels, closed form -----------------------------------------------------------------------------------------------

def basis_rho_vec(W, i):
    v = np.zeros(1 << (2 * W), dtype=np.complex128)
    v[i | (i << W)] = 1.0
    return v


@pytest.mark.parametrize("W", [1, 4, 7])
def test_forced_kraus_channels_end_in_their_basis_state(W):
    with _lib.Engine(2 * W) as eng:
        for label, (rec, data), want in kc.forced_programs(W):
            eng.density_exec(rec, data)
            err = float(np.abs(eng.amplitudes() - basis_rho_vec(W, want)).max())
            assert err <= AMP_TOL, (label, err)


@pytest.mark.parametrize("W", [2, 6])
def test_probability_one_paulis(W):
    bad = []
    with _lib.Engine(2 * W) as eng:
        for qs, p in nc.forced_pauli_cases(W):
            for (rec, data), want in nc.forced_pauli_programs(W, list(qs), p):
                eng.density_exec(rec, data)
                err = float(np.abs(eng.amplitudes() - basis_rho_vec(W, want)).max())
                if err > AMP_TOL:
                    bad.append((qs, p, want, err))
    assert not bad, bad


def test_refusals():
    rng = np.random.RandomState(1)
    with _lib.Engine(5) as odd:
        with pytest.raises(ValueError, match="2W"):
            odd.density_exec(*program.encode([ir.op_x(0)]))
    with _lib.Engine(6) as eng:
        eng.density_exec(*program.encode([ir.op_x(1)]))
        before = eng.amplitudes()
        for ops in ([ir.op_x(3)], [ir.op_x(0, [3], [1])], [ir.op_diag([0, 4], np.ones(4))], [nc._pauli(rng, [3])],
                    [ir.op_x(0), kc.kraus_op(3, kc.isometry_kraus(rng, 2))]):
            with pytest.raises(ValueError, match="density matrix"):
                eng.density_exec(*program.encode(ops))
        rec, data = program.encode([kc.kraus_op(0, kc.isometry_kraus(rng, 2))])
        rec["vals"][0, 0] = 5
        with pytest.raises(ValueError, match="1 to 4 operators"):
            eng.density_exec(rec, data)
        rec, data = program.encode([nc._pauli(rng, [0, 1])])
        rec["n"][0] = 3
        with pytest.raises(ValueError, match="1 or 2 qubits"):
            eng.density_exec(rec, data)
        for kind in (_lib.OP_MUX, _lib.OP_KQ, _lib.OP_SWAP):
            rec, data = program.encode([ir.op_x(0)])
            rec["kind"][0] = kind
            with pytest.raises(RuntimeError, match=r"\(-5\)"):
                eng.density_exec(rec, data)
        assert np.array_equal(eng.amplitudes(), before)              # a refused program leaves the state as it was
        with pytest.raises(ValueError):
            eng.density_diagonal([0, 1, 2, 0])
        with pytest.raises(ValueError, match="qsv_noisy_sample only"):   # qsv_exec goes on refusing the channel kinds
            eng.exec(*program.encode([nc._pauli(rng, [0])]))
    with _lib.Engine(6, devices=(0, 0)) as two:
        with pytest.raises(RuntimeError, match=r"\(-5\)"):
            two.density_exec(*program.encode([ir.op_x(0)]))


# ---- large and cheap: products of pair factors -------------------------------------------------------------------------------------

@pytest.mark.parametrize("W", [12, 13])
def test_pair_product_program(W):
    ops, factors = dc.pair_program(W)
    rec, data = program.encode(ops)
    diag = dc.product_diagonal(factors, W)
    rng = np.random.RandomState(W)
    with _lib.Engine(2 * W) as eng:
        eng.density_exec(rec, data)
        for qs in ([0, W - 1, 5, 6, W - 2, 7], [int(q) for q in rng.permutation(W)[:10]], [3]):
            m, trace = eng.density_diagonal(qs)
            assert abs(trace - 1.0) <= AMP_TOL
            assert np.abs(m - dc.marginal(diag, qs)).max() <= PROB_TOL, qs
        worst = 0.0
        for j in (0, 1, (1 << W) - 1, int(rng.randint(1 << W)), 1 << (W - 1) | 1 << 5):
            row = eng.amplitudes(j << W, 1 << W)                     # rho[:, j]
            want = dc.product_entries(factors, W, np.arange(1 << W), np.full(1 << W, j))
            worst = max(worst, float(np.abs(row - want).max()))
        print("DENSITY pair product W=%d: max |amp - reference| over 5 columns = %.3g, |trace - 1| = %.3g" % (W, worst, abs(trace - 1.0)))
        assert worst <= AMP_TOL


# ---- sampling, word by word -----------------------------------------------------------------------------------------------------

def sampled(eng, c, shots=None):
    return eng.density_sample(c["shots"] if shots is None else shots, c["seed"], c["meas"], c["readout"])


@pytest.mark.parametrize("name", [n for n in dc.SAMPLE_CASES if n != "prefix of 6000"])
def test_density_sample_every_word(name):
    c = dc.sample_case(name)
    words, alt, amb, diag = dc.sample_reference(name)
    with _lib.Engine(2 * c["W"]) as eng:
        eng.density_exec(c["rec"], c["data"])
        got = sampled(eng, c)
        full, _ = eng.density_diagonal(list(range(c["W"])))
    assert np.abs(full - diag).max() <= PROB_TOL
    nc.check_words(got, words, alt, amb, family="density sample", label=name)


def test_prefix_of_a_larger_call_and_the_full_index():
    small, big = kc.seed_case(kc.BIG_SEEDS[0]), dc.sample_case("prefix of 6000")
    words, alt, amb, diag = dc.sample_reference("prefix of 6000")
    with _lib.Engine(2 * big["W"]) as eng:
        eng.density_exec(big["rec"], big["data"])
        all6000 = sampled(eng, big)
        first = sampled(eng, big, small["shots"])
        idx = eng.density_sample(500, 99)                            # no register: the full basis index
        none = eng.density_sample(0, 99)
    nc.check_words(all6000, words, alt, amb, family="density sample", label="6000 shots")
    assert np.array_equal(all6000[:small["shots"]], first)           # a shot depends on (seed, shot) alone
    want = dc.exact_density_sample(diag, 500, 99)
    nc.check_words(idx, *want, family="density sample", label="full index")
    assert idx.max() < 1 << big["W"] and none.size == 0


def test_noise_free_program_samples_as_the_trajectory_kernel_does():
    c = dc.sample_case("noise free")
    words, alt, amb, _ = dc.sample_reference("noise free")
    with _lib.Engine(2 * c["W"]) as eng:
        eng.density_exec(c["rec"], c["data"])
        a = sampled(eng, c)
    with _lib.Engine(c["W"]) as eng:
        b = eng.noisy_sample(c["rec"], c["data"], c["shots"], c["seed"], c["meas"], c["readout"])
    differ = np.flatnonzero(a != b)
    print("DENSITY noise free: %d of %d words differ between density_sample and noisy_sample, %d ambiguous" % (differ.size, a.size, int(amb.sum())))
    assert int(amb.sum()) <= nc.ambiguity_cap(a.size)
    assert amb[differ].all()                                         # only where the draw sits on a boundary
    for i in differ:
        assert {int(a[i]), int(b[i])} == {int(words[i]), int(alt[i])}


# ---- end to end ------------------------------------------------------------------------------------------------------------------

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


def as_array(probs, nbits):
    out = np.zeros(1 << nbits)
    for k, v in probs.items():
        out[int(k.replace(" ", ""), 2)] = v
    return out


def circuits():
    g = nc.models_05()
    yield "lowered graph 1", transpile(QCMRF(g["GRAPHS"][1], g["THETAS"]["1"][2], with_measurements=True), basis_gates=nc.BASIS), kc.thermal_model()
    yield "constructed graph 2", QCMRF(g["GRAPHS"][2], g["THETAS"]["2"][4], with_measurements=True), kc.constructed_model()


@pytest.mark.parametrize("which", [0, 1])
def test_run_density_matrix_end_to_end(be, which):
    label, qc, nm = list(circuits())[which]
    want = exact(qc, nm)
    res = be.run(qc, shots=SHOTS, seed_simulator=900 + which, method="density_matrix", noise_model=nm).result()
    probs, counts, meta = res.get_probabilities(), res.get_counts(), res.metadata(0)
    own = as_array(probs, qc.num_clbits)
    print("DENSITY %s: max |p - reference| = %.3g, |trace - 1| = %.3g, %d pauli, %d kraus records" % (
        label, np.abs(own - want).max(), abs(meta["trace"] - 1.0), meta["n_pauli_ops"], meta["n_kraus_ops"]))
    assert meta["method"] == "density_matrix" and meta["n_kraus_ops"] > 0 and abs(meta["trace"] - 1.0) <= AMP_TOL
    assert np.abs(own - want).max() <= PROB_TOL and abs(own.sum() - 1.0) <= 1e-12
    assert sum(counts.values()) == SHOTS
    assert chi2_pvalue(counts, own, SHOTS) > 1e-4
    assert chi2_pvalue(counts, want, SHOTS) > 1e-4
    assert be.run(qc, shots=SHOTS, seed_simulator=900 + which, method="density_matrix", noise_model=nm).result().get_counts() == counts
    # the trajectory path's shots of the same circuit against the device's exact distribution
    noisy = be.run(qc, shots=SHOTS, seed_simulator=950 + which, noise_model=nm).result()
    assert noisy.metadata(0)["method"] == "noisy"
    assert chi2_pvalue(noisy.get_counts(), own, SHOTS) > 1e-4


def test_success_rates_of_damping_and_its_twirl_as_exact_numbers(be):
    T, n = kc.success_circuit()
    rates = []
    for nm in kc.success_models(0.2):
        probs = be.run(T, shots=0, method="density_matrix", noise_model=nm).result().get_probabilities()
        got, want = kc.success_rate(as_array(probs, T.num_clbits), n), kc.success_rate(exact(T, nm), n)
        assert abs(got - want) <= PROB_TOL
        rates.append(got)
    print("DENSITY success rate: damping %.12f, Pauli twirl %.12f" % tuple(rates))
    assert abs(rates[0] - 0.61) < 0.005 and abs(rates[1] - 0.49) < 0.005
    assert rates[0] > rates[1]


def test_an_ideal_run_gives_the_closed_form(be):
    from oracle import closed_form as cf
    g = nc.models_05()
    C, th = g["GRAPHS"][2], g["THETAS"]["2"][4]
    res = be.run(QCMRF(C, th, with_measurements=True), shots=100, seed_simulator=4, method="density_matrix").result()
    got = as_array(res.get_probabilities(), 8)
    assert np.abs(got - cf.probabilities(C, th)).max() <= PROB_TOL
    with pytest.raises(ValueError, match="unknown method"):
        be.run(QCMRF(C, th, with_measurements=True), shots=1, method="tensor_network")
