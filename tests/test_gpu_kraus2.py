"""Two-qubit Kraus channels on the MI355X beyond single words: ``qsv_density_exec`` on KRAUS2 records against the numpy
walker (amplitudes within 1e-12, probabilities within 1e-10: the file-wide promises of test_gpu_density.py), trajectories
against the density matrix, ``run()`` in its modes, the effect the record exists for -- a coherent error is not its Pauli
twirl --, and the refusals."""
import numpy as np
import pytest

import _kraus2_cases as k2c
import _noise_exact_cases as nc
from _density_cases import marginal, vec_of
from _density_matrix import chi2_pvalue
from _kraus2_reference import kraus2_rho
from qcmrf_amd import _lib, ir, program
from qcmrf_amd.backend import QsvBackend
from qcmrf_amd.noise import NoiseModel, thermal_relaxation_error, two_qubit_kraus_error

pytestmark = pytest.mark.gpu

AMP_TOL, PROB_TOL = 1e-12, 1e-10
SHOTS = 20000


@pytest.fixture(scope="module")
def be():
    b = QsvBackend()
    yield b
    b.close()


def density_program(W, pair, stack, rng):
    """a generic state (a layer of unitaries and an entangler), then one KRAUS2 record on ``pair``, then another layer"""
    a, b = pair
    ops = [ir.op_u(q, nc._unitary(rng)) for q in range(W)] + [ir.op_x(a, [b], [1])]
    if W > 2:
        ops.append(ir.op_x((a + 1) % W if (a + 1) % W != b else (b + 1) % W, [a], [1]))
    ops.append(k2c.kraus2_op(a, b, stack))
    ops += [ir.op_u(q, nc._unitary(rng)) for q in (a, b)]
    return program.encode(ops)


# ---- the density matrix, record level -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("W", [2, 3, 5, 9])
def test_density_exec_on_kraus2_records(W):
    """every pair placement ((q, q + W) strides included: the bra bits of the pair sit W above its ket bits), every stack of
    the menu; whole vector, trace and Hermiticity"""
    rng = np.random.RandomState(900 + W)
    stacks = k2c.menu(rng)
    worst = 0.0
    with _lib.Engine(2 * W) as eng:
        for i, pair in enumerate(k2c.pairs(W) * (2 if W < 5 else 1)):
            rec, data = density_program(W, pair, stacks[(3 * i + W) % len(stacks)], rng)
            rho = kraus2_rho(rec, data, W)
            eng.density_exec(rec, data)
            got = eng.amplitudes()
            err = float(np.abs(got - vec_of(rho)).max())
            G = got.reshape(1 << W, 1 << W).T
            full, trace = eng.density_diagonal(list(range(W)))
            worst = max(worst, err)
            assert err <= AMP_TOL, (pair, err)
            assert float(np.abs(G - G.conj().T).max()) <= AMP_TOL and abs(trace - 1.0) <= AMP_TOL, pair
            assert np.abs(full - np.real(np.diag(rho))).max() <= PROB_TOL, pair
            m, _ = eng.density_diagonal([pair[1], pair[0]])
            assert np.abs(m - marginal(np.real(np.diag(rho)), [pair[1], pair[0]])).max() <= PROB_TOL
    print("DENSITY kraus2 W=%d: max |amp - reference| = %.3g" % (W, worst))


@pytest.mark.parametrize("W", [3, 7])
def test_density_exec_on_a_whole_random_program(W):
    c = k2c.case("W=%d" % W)
    rho = kraus2_rho(c["rec"], c["data"], W)
    with _lib.Engine(2 * W) as eng:
        eng.density_exec(c["rec"], c["data"])
        assert float(np.abs(eng.amplitudes() - vec_of(rho)).max()) <= AMP_TOL


def test_product_channel_given_densely_gives_the_distribution_of_the_product_form(be):
    t = thermal_relaxation_error(20e3, 30e3, 1500.0)
    dense = two_qubit_kraus_error([np.kron(b, a) for a in t.kraus() for b in t.kraus()])
    T = k2c.chain3(True)
    probs = []
    for e in (t.expand(t), dense):
        nm = NoiseModel()
        nm.add_all_qubit_quantum_error(e, ["cx"])
        res = be.run(T, shots=100, seed_simulator=3, noise_model=nm, method="density_matrix").result()
        probs.append(res.get_probabilities())
        assert (res.metadata(0)["n_kraus2_ops"] > 0) == (e is dense)
    keys = set(probs[0]) | set(probs[1])
    assert max(abs(probs[0].get(k, 0.0) - probs[1].get(k, 0.0)) for k in keys) <= PROB_TOL


# ---- trajectories against the density matrix ----------------------------------------------------------------------------------

@pytest.mark.parametrize("state", ["lds", "hbm"])
def test_trajectories_against_the_density_matrix(be, state):
    T, nm = k2c.chain3(True), k2c.lowered_model()
    exact = k2c.exact_distribution(T, nm)
    res = be.run(T, shots=SHOTS, seed_simulator=811, noise_model=nm, noisy_state=state).result()
    counts, meta = res.get_counts(), res.metadata(0)
    assert sum(counts.values()) == SHOTS and meta["method"] == "noisy" and meta["n_kraus2_ops"] > 0
    p_fit, p_ideal = chi2_pvalue(counts, exact, SHOTS), chi2_pvalue(counts, k2c.exact_distribution(T, None), SHOTS)
    print("KRAUS2 chi2 (%s): p(density matrix) = %.3g, p(ideal) = %.3g, %d kraus2 ops" % (state, p_fit, p_ideal, meta["n_kraus2_ops"]))
    assert p_fit > 1e-4
    assert p_ideal < 1e-12


@pytest.mark.parametrize("options", [dict(noisy_state="auto"), dict(noisy_measure="in_place"), dict(noisy_measure="auto"),
                                     dict(noisy_measure="in_place", accept={4: 0, 5: 0})])
def test_run_modes(be, options):
    """the remaining modes of run(): counts against the exact (for accept: the conditioned) distribution"""
    T, nm = k2c.chain3(True), k2c.lowered_model()
    exact = k2c.exact_distribution(T, nm)
    if "accept" in options:
        keep = np.array([(w >> 3) == 0 for w in range(exact.size)])
        exact = np.where(keep, exact, 0.0) / exact[keep].sum()
    res = be.run(T, shots=4000, seed_simulator=812, noise_model=nm, **options).result()
    counts = res.get_counts()
    assert sum(counts.values()) == 4000 and res.metadata(0)["n_kraus2_ops"] > 0
    assert chi2_pvalue(counts, exact, 4000) > 1e-4


# ---- the effect: a coherent over-rotation is not its Pauli twirl ----------------------------------------------------------------

def test_coherent_error_moves_the_result_more_than_its_pauli_twirl(be):
    """exact density-matrix probabilities on the lowered chain of 3 variables: the ZX over-rotation behind every cx changes
    the post-selected distribution and the all-ancillas-zero rate by more than the Pauli error of the same process fidelity:
    its amplitudes add across the compute and uncompute blocks, the twirl's probabilities do not.  The expected values
    are the numpy walker's."""
    T = k2c.chain3(True)
    want = k2c.effect_expected()
    coh, twirl = k2c.coherent_and_twirl()
    got = {}
    for name, nm in (("ideal", None), ("coherent", coh), ("twirl", twirl)):
        extra = {} if nm is None else {"noise_model": nm}
        probs = be.run(T, shots=10, seed_simulator=1, method="density_matrix", **extra).result().get_probabilities()
        dist = np.zeros(1 << len(next(iter(probs)).replace(" ", "")))
        for k, v in probs.items():
            dist[int(k.replace(" ", ""), 2)] = v
        got[name] = k2c.post_selected(dist, 3)
        assert np.abs(got[name][0] - want[name][0]).max() <= PROB_TOL and abs(got[name][1] - want[name][1]) <= PROB_TOL, name
    tv = {n: 0.5 * np.abs(got[n][0] - got["ideal"][0]).sum() for n in ("coherent", "twirl")}
    dr = {n: abs(got[n][1] - got["ideal"][1]) for n in ("coherent", "twirl")}
    print("KRAUS2 effect: post-selected TV distance coherent %.5f, twirl %.5f; success rate ideal %.5f, coherent %.5f, twirl %.5f"
          % (tv["coherent"], tv["twirl"], got["ideal"][1], got["coherent"][1], got["twirl"][1]))
    assert tv["coherent"] > tv["twirl"]
    assert dr["coherent"] > dr["twirl"]


# ---- refusals -------------------------------------------------------------------------------------------------------------------

def test_malformed_records_and_exec_refuse():
    rng = np.random.RandomState(8)
    ks = k2c.isometry_kraus2(rng, 2)
    rec, data = program.encode([k2c.kraus2_op(0, 2, ks)])

    def changed(**fields):
        r = rec.copy()
        for k, v in fields.items():
            if k == "q":
                r["qubits"][0, :2] = v
            elif k == "m":
                r["vals"][0, 0] = v
            else:
                r[k] = v
        return r

    with _lib.Engine(3) as eng:
        assert eng.noisy_sample(rec, data, 8, 1).shape == (8,)
        for bad in (changed(q=(1, 1)), changed(m=0), changed(m=17), changed(q=(0, 3)), changed(q=(3, 0)), changed(n=1)):
            for fn in (eng.noisy_sample, eng.noisy_sample_hbm):
                with pytest.raises(ValueError, match="KRAUS2"):
                    fn(bad, data, 8, 1)
            with pytest.raises(ValueError, match="KRAUS2"):
                eng.noisy_sample_accept(bad, data, 8, 1)
        with pytest.raises(ValueError, match="KRAUS2"):
            eng.noisy_sample(rec, np.where(np.arange(data.size) == 64, 0.5, data), 8, 1)      # E tables no longer sum to 1
        with pytest.raises(ValueError, match="KRAUS2"):
            eng.exec(rec, data)
    with _lib.Engine(6) as eng:
        for bad in (changed(q=(1, 1)), changed(m=17), changed(q=(0, 3))):
            with pytest.raises(ValueError, match="KRAUS2"):
                eng.density_exec(bad, data)
