"""``run(..., noise_model=nm, accept={classical bit: 0 | 1})`` on the host: the option, its metadata, its refusals and its
determinism with a Philox-exact stand-in for the engine (_accept_cases.AcceptExactEngine: ``noisy_sample_accept`` from
``exact_measure_sample(first_shot=...)``); ``method='density_matrix'`` with ``accept`` against the numpy density references;
and, for every seeded case the GPU tests run, that the reference alone stays within the project's ambiguity cap."""
import numpy as np
import pytest

import _accept_cases as ac
import _kraus_cases as kc
import _measure_cases as mc
from _density_cases import DensityNumpyEngine
from _density_matrix import chi2_pvalue
from _kraus_reference import kraus_density_distribution, within_cap
from _measure_reference import measure_density_distribution
from qcmrf_amd import QCMRF
from qcmrf_amd.backend import QsvBackend
from qcmrf_amd.noise import NoiseModel


def backend(engine=ac.AcceptExactEngine, **options):
    b = QsvBackend(**options)
    b._engine_factory = lambda n, devices=(0,), rank=None, world_size=None: engine(n, len(devices))
    return b


def density_backend():
    b = QsvBackend()
    b._engine_factory = DensityNumpyEngine
    return b


def chain(n):
    qc = QCMRF(mc.chain(n), mc.chain_theta(n), with_measurements=True)
    return mc.chain_circuit(n), qc.post_selection()


def filtered(counts, fixed):
    return {k: v for k, v in counts.items() if all(k.replace(" ", "")[::-1][c] == str(b) for c, b in fixed.items())}


@pytest.fixture(scope="module")
def chain3_run():
    qc, fixed = chain(3)
    nm = kc.thermal_model()
    res = backend().run(qc, shots=120, seed_simulator=77, noise_model=nm, noisy_measure="in_place", accept=fixed).result()
    return qc, nm, fixed, res


# ---- the option ---------------------------------------------------------------------------------------------------------------

def test_counts_carry_the_fixed_bits_and_sum_to_shots(chain3_run):
    qc, nm, fixed, res = chain3_run
    counts, m = res.get_counts(), res.metadata()
    assert fixed == {4: 0, 5: 0}
    assert sum(counts.values()) == 120 and filtered(counts, fixed) == counts
    assert m["accept"] == fixed and m["method"] == "noisy" and m["noisy_measure"] == "in_place"
    assert m["accept_attempts"] >= 120
    assert m["accept_probability"] == pytest.approx(119 / (m["accept_attempts"] - 1))
    print("chain(3) lowered, thermal model: 120 shots accepted in %d attempts" % m["accept_attempts"])


@pytest.mark.parametrize("measure,state", [("in_place", "lds"), ("deferred", "lds"), ("auto", "hbm")])
def test_accept_is_the_filtered_plain_run(chain3_run, measure, state):
    """the first ``shots`` accepted attempts are the accepted shots of the plain run of ``accept_attempts`` shots"""
    qc, nm, fixed, res = chain3_run
    b = backend()
    got = b.run(qc, shots=120, seed_simulator=77, noise_model=nm, noisy_measure=measure, noisy_state=state, accept=fixed).result()
    m = got.metadata()
    base = b.run(qc, shots=m["accept_attempts"], seed_simulator=77, noise_model=nm, noisy_measure=measure, noisy_state=state).result()
    assert filtered(base.get_counts(), fixed) == got.get_counts()
    assert m["noisy_state"] == state and sum(got.get_counts().values()) == 120


def test_nothing_depends_on_the_round(chain3_run):
    qc, nm, fixed, res = chain3_run
    for n in (1, 7, 64, 0):
        ac.AcceptExactEngine.rounds.clear()
        got = backend().run(qc, shots=120, seed_simulator=77, noise_model=nm, noisy_measure="in_place", accept=fixed,
                            accept_round=n).result()
        assert got.get_counts() == res.get_counts(), n
        assert got.metadata()["accept_attempts"] == res.metadata()["accept_attempts"]
        assert n == 0 or set(ac.AcceptExactEngine.rounds) <= {n}, "accept_round did not reach the engine"


def test_one_dict_per_circuit_and_one_seed_per_circuit():
    qa, fa = chain(3)
    qb, fb = chain(2)
    nm = kc.thermal_model()
    b = backend()
    both = b.run([qa, qb], shots=40, seed_simulator=9, noise_model=nm, noisy_measure="in_place", accept=[fa, fb]).result()
    assert [both.metadata(i)["accept"] for i in (0, 1)] == [fa, fb] and fa != fb
    one = b.run(qb, shots=40, seed_simulator=10, noise_model=nm, noisy_measure="in_place", accept=fb).result()        # seed + i
    assert one.get_counts() == both.get_counts()[1] and one.metadata()["accept_attempts"] == both.metadata(1)["accept_attempts"]
    same = b.run([qa, qa], shots=40, seed_simulator=9, noise_model=nm, noisy_measure="in_place", accept=fa).result()   # one dict for all
    assert same.get_counts()[0] == both.get_counts()[0] and same.get_counts()[1] != same.get_counts()[0]
    with pytest.raises(ValueError, match="one per circuit"):
        b.run([qa, qb], shots=40, noise_model=nm, accept=[fa])
    with pytest.raises(ValueError, match="one per circuit"):
        b.run(qa, shots=40, noise_model=nm, accept=[4, 5])


def test_one_shot_estimate():
    qc, fixed = chain(2)
    m = backend().run(qc, shots=1, seed_simulator=3, noise_model=kc.thermal_model(), accept=fixed).result().metadata()
    assert m["accept_probability"] == 1.0 / m["accept_attempts"]


def test_running_out_of_attempts_is_a_runtime_error():
    qc, fixed = chain(3)
    with pytest.raises(RuntimeError, match=r"25 attempts made, \d+ of 120 shots accepted \(rate seen 0\.\d+\)"):
        backend().run(qc, shots=120, seed_simulator=77, noise_model=kc.thermal_model(), noisy_measure="in_place", accept=fixed,
                      accept_max_attempts=25)


def test_refusals():
    qc, fixed = chain(3)
    nm = kc.thermal_model()
    b = backend()
    with pytest.raises(ValueError, match="both"):
        b.run(qc, shots=10, noise_model=nm, accept=fixed, post_select=fixed)
    with pytest.raises(ValueError, match="both"):
        b.run(qc, shots=10, accept=fixed, post_select=fixed)
    with pytest.raises(ValueError, match="post_select"):               # an ideal run: no model ...
        b.run(qc, shots=10, accept=fixed)
    with pytest.raises(ValueError, match="post_select"):               # ... or an empty one
        b.run(qc, shots=10, noise_model=NoiseModel(), accept=fixed)
    with pytest.raises(ValueError, match="trajectory"):
        b.run(qc, shots=10, accept=fixed, method="trajectory")
    with pytest.raises(ValueError, match="trajectory"):
        b.run(qc, shots=10, noise_model=nm, accept=fixed, method="trajectory")

    class Ranks:
        world, rank = 2, 0
    with pytest.raises(ValueError, match="one process"):
        b.run(qc, shots=10, noise_model=nm, accept=fixed, comm=Ranks())
    with pytest.raises(ValueError, match="no measurement writes"):
        b.run(qc, shots=10, noise_model=nm, accept={17: 0})
    with pytest.raises(ValueError, match="0 or 1"):
        b.run(qc, shots=10, noise_model=nm, accept={4: 2})
    # post_select keeps refusing what it refused
    with pytest.raises(ValueError, match="noise_model"):
        b.run(qc, shots=10, noise_model=nm, post_select=fixed)


# ---- method='density_matrix' --------------------------------------------------------------------------------------------------

def two_cliques_on_a_pair():
    """2 variables, 2 cliques: 5 qubits"""
    from qcmrf_amd.transpile import transpile
    import _noise_exact_cases as nc
    qc = QCMRF([[0, 1], [0, 1]], mc.chain_theta(3), with_measurements=True)
    return transpile(qc, basis_gates=nc.BASIS), qc.post_selection()


@pytest.mark.parametrize("name,model", [("chain(2)", "thermal"), ("pair twice", "thermal"), ("chain(3)", "thermal"),
                                        ("chain(3)", "readout only")])
def test_density_conditioned_distribution(name, model):
    """4 to 6 qubit circuits: the conditioned distribution, readout confusion included, is the numpy reference's, conditioned
    and renormalised; accept_probability is the mass of the condition; the counts are one multinomial draw"""
    qc, fixed = {"chain(2)": lambda: chain(2), "pair twice": two_cliques_on_a_pair, "chain(3)": lambda: chain(3)}[name]()
    nm = kc.thermal_model() if model == "thermal" else mc.local_readout_model(NoiseModel(), 6)
    res = density_backend().run(qc, shots=500, seed_simulator=21, noise_model=nm, method="density_matrix", accept=fixed).result()
    ing, rec, data, clist, meas, readout, _ = QsvBackend._prepare_density(qc, nm)
    assert ing.num_qubits == {"chain(2)": 4, "pair twice": 5, "chain(3)": 6}[name]
    full = kraus_density_distribution(rec, data, ing.num_qubits, meas, readout if ing.readout else None)
    assert np.allclose(full, measure_density_distribution(rec, data, ing.num_qubits, meas, readout if ing.readout else None), atol=1e-13)
    keep = ac.accepts(np.arange(full.size, dtype=np.uint64), fixed)
    mass = full[keep].sum()
    want = np.where(keep, full, 0.0) / mass
    probs = res.get_probabilities()
    got = np.zeros(full.size)
    for k, v in probs.items():
        got[int(k.replace(" ", ""), 2)] = v
    assert np.abs(got - want).max() < 1e-12 and filtered(probs, fixed) == probs
    m = res.metadata()
    assert m["accept"] == fixed and m["accept_probability"] == pytest.approx(mass, abs=1e-12) and 0.0 < mass < 1.0
    counts = res.get_counts()
    idx = np.flatnonzero(got > 0)
    drawn = np.random.default_rng(21).multinomial(500, got[idx] / got[idx].sum())
    assert {int(k.replace(" ", ""), 2): v for k, v in counts.items()} == {int(i): int(c) for i, c in zip(idx, drawn) if c}


def test_density_zero_mass_is_post_selects_error():
    """a qubit nothing acts on reads 0 for certain"""
    from qcmrf_amd.circuit import QuantumCircuit
    qz = QuantumCircuit(2, 2)
    qz.h(0)
    qz.measure(0, 0)
    qz.measure(1, 1)
    b = density_backend()
    with pytest.raises(ValueError, match="zero probability"):
        b.run(qz, shots=10, method="density_matrix", accept={1: 1})
    res = b.run(qz, shots=10, seed_simulator=2, method="density_matrix", accept={1: 0}).result()
    assert res.metadata()["accept_probability"] == pytest.approx(1.0) and sum(res.get_counts().values()) == 10


def test_trajectory_counts_against_the_conditioned_distribution():
    """the stand-in engine is exact shot by shot, so its accepted counts follow the conditioned exact distribution, and the
    exact success probability lies inside the interval its attempts give"""
    from scipy.stats import beta
    qc, fixed = chain(3)
    nm, shots = kc.thermal_model(), 600
    res = backend().run(qc, shots=shots, seed_simulator=5, noise_model=nm, noisy_measure="in_place", accept=fixed).result()
    exact = density_backend().run(qc, shots=1, seed_simulator=5, noise_model=nm, method="density_matrix", accept=fixed).result()
    dist = np.zeros(64)
    for k, v in exact.get_probabilities().items():
        dist[int(k.replace(" ", ""), 2)] = v
    p = chi2_pvalue(res.get_counts(), dist, shots)
    attempts, rate = res.metadata()["accept_attempts"], exact.metadata()["accept_probability"]
    lo, hi = beta.ppf(0.5e-4, shots, attempts - shots + 1), beta.ppf(1 - 0.5e-4, shots + 1, attempts - shots)
    print("accept (stand-in) against the conditioned exact distribution: p = %.3g; rate %.4f in [%.4f, %.4f], %d attempts"
          % (p, rate, lo, hi, attempts))
    assert p > 1e-4 and lo <= rate <= hi


# ---- the seeded cases of the GPU tests ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(ac.PLANS))
def test_gpu_cases_stay_within_the_ambiguity_cap(name):
    """the reference alone: flagged shots of the window within the cap, none among the attempts a call examines (the GPU
    test asserts ``attempts`` exactly), the call ends inside the window, and both outcomes occur among the examined"""
    path, choices = ac.PLANS[name]
    sizes = set()
    for fixed in choices:
        p = ac.plan(name, fixed)
        words, alt, amb, undet = p["ref"]
        n, cap = within_cap(amb, undet)
        assert n <= cap, "%s: %d flagged shots of %d (cap %d)" % (name, n, words.size, cap)
        assert p["flagged_examined"] == 0, "%s %r: a flagged shot among the %d examined attempts" % (name, fixed, p["attempts"])
        assert words.size <= 2000 and p["shots"] <= p["attempts"] < words.size
        rejected = p["attempts"] - p["shots"]
        assert rejected >= p["attempts"] // 10, "%s %r rejects too little to test anything" % (name, fixed)
        sizes.add(len(fixed))
        # the stand-in engine implements the same rule by rounds: the same answer
        c = p["case"]
        eng = ac.AcceptExactEngine(c["W"], 1)
        fm, fv = ac.mask_of(fixed)
        if c["W"] <= 8:
            got = eng.noisy_sample_accept(c["rec"], c["data"], p["shots"], c["seed"], c["meas"], c["readout"], fm, fv,
                                          max_attempts=words.size, round=257, hbm=path == "hbm")
            ac.check_accept(got, p, name + " stand-in")
    assert len(sizes) >= 1
    bits = {b for _, cs in ac.PLANS.values() for f in cs for b in f}
    vals = {v for _, cs in ac.PLANS.values() for f in cs for v in f.values()}
    assert 63 in bits and vals == {0, 1} and {len(f) for _, cs in ac.PLANS.values() for f in cs} == {1, 2, 3}


# ---- run_experiment -----------------------------------------------------------------------------------------------------------

def test_run_experiment_post_select_with_noise_uses_accept(tmp_path, monkeypatch):
    import json
    from qcmrf_amd import backend as be_mod, run_experiment
    import qcmrf_amd.workloads as wl
    monkeypatch.setattr(wl, "REFERENCE_GRAPHS", wl.REFERENCE_GRAPHS[:2])
    graphs = wl.REFERENCE_GRAPHS
    b = backend()
    monkeypatch.setattr(be_mod.Aer, "get_backend", lambda name="qasm_simulator", **o: b)
    args = ["--scale", "0.5", "--shots", "30", "--reps", "1", "--outdir", str(tmp_path), "--seed-simulator", "5", "--post-select",
            "--depolarizing", "0.001,0.01", "--readout", "0.02"]
    counts = run_experiment.main(args + ["--noisy-measure", "auto"])
    assert json.load(open(tmp_path / "result_simulation_noisy_postselected_0.5.json")) == counts
    rates = json.load(open(tmp_path / "success_simulation_noisy_0.5.json"))
    assert len(counts) == len(rates) == 2 and all(0.0 < r <= 1.0 for r in rates)
    for C, c in zip(graphs, counts):
        assert sum(c.values()) == 30 and all(k[:len(C)] == "0" * len(C) for k in c)
    d = density_backend()
    monkeypatch.setattr(be_mod.Aer, "get_backend", lambda name="qasm_simulator", **o: d)
    run_experiment.main(args + ["--method", "density_matrix"])
    exact = json.load(open(tmp_path / "success_simulation_noisy_0.5.json"))
    probs = json.load(open(tmp_path / "probs_simulation_noisy_0.5.json"))
    assert rates != exact and all(abs(sum(p.values()) - 1.0) < 1e-12 for p in probs)
    assert all(k[:len(C)] == "0" * len(C) for C, p in zip(graphs, probs) for k in p)
