"""The references of the Kraus tests, tested on the host: the density-matrix walker against closed forms, the
Philox-exact per-shot reference against the density matrix, the ambiguity cap of every device case on the reference
alone, and the comparison helper against references made wrong the way a kernel could be."""
import numpy as np
import pytest

import _kraus_cases as kc
import _noise_exact_cases as nc
from _density_matrix import chi2_pvalue
from _kraus_reference import (MUTATIONS, check_kraus_words, exact_kraus_sample, kraus_density_distribution, kraus_of_record,
                              kraus_step, within_cap)
from qcmrf_amd import _lib, ir, program
from qcmrf_amd.noise import amplitude_damping_error, reset_error, thermal_relaxation_error

_H = np.array([[1, 1], [1, -1]], dtype=np.complex128) / np.sqrt(2.0)


def stack(err):
    return np.array(err.kraus())


# ---- the density-matrix walker --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("gamma", [0.0, 0.2, 0.75, 1.0])
def test_density_matrix_damping_after_x(gamma):
    """damping gamma on X|0>: P(1) = 1 - gamma"""
    rec, data = program.encode([ir.op_x(1), kc.kraus_op(1, stack(amplitude_damping_error(gamma)))])
    p = kraus_density_distribution(rec, data, 2, [1])
    assert np.allclose(p, [gamma, 1.0 - gamma], atol=1e-15)


def test_density_matrix_reset_after_h_gives_zero():
    rec, data = program.encode([ir.op_u(0, _H), ir.op_u(2, _H), ir.op_x(1, [0]), kc.kraus_op(0, stack(reset_error(1.0)))])
    p = kraus_density_distribution(rec, data, 3, [0, 1, 2])
    want = np.zeros(8)
    want[[0b000, 0b010, 0b100, 0b110]] = 0.25                       # qubit 0 back in |0>, its partner left mixed
    assert np.allclose(p, want, atol=1e-15)
    rec, data = program.encode([ir.op_u(0, _H), kc.kraus_op(0, stack(reset_error(0.0, 1.0)))])
    assert np.allclose(kraus_density_distribution(rec, data, 1, [0]), [0.0, 1.0], atol=1e-15)


def test_density_matrix_thermal_populations_and_coherence():
    """H|0> under thermal relaxation, then H: P(0) = (1 + e2) / 2 whatever t1 does to the populations of a uniform state"""
    t1, t2, time = 100.0, 150.0, 30.0
    rec, data = program.encode([ir.op_u(0, _H), kc.kraus_op(0, stack(thermal_relaxation_error(t1, t2, time))), ir.op_u(0, _H)])
    p = kraus_density_distribution(rec, data, 1, [0])
    assert np.allclose(p[0], 0.5 * (1.0 + np.exp(-time / t2)), atol=1e-14)
    rec, data = program.encode([ir.op_x(0), kc.kraus_op(0, stack(thermal_relaxation_error(t1, t2, time, 0.25)))])
    p = kraus_density_distribution(rec, data, 1, [0])
    assert np.allclose(p[0], 0.75 * (1.0 - np.exp(-time / t1)), atol=1e-14)


# ---- one step of the contract ----------------------------------------------------------------------------------------------

def test_kraus_step_keeps_the_mass_and_picks_by_cumulative_weight():
    rng = np.random.RandomState(2)
    W, S = 3, 9
    psi = rng.randn(1 << W, S) + 1j * rng.randn(1 << W, S)
    psi *= rng.uniform(0.5, 2.0, S)                                 # unnormalised: weights are relative to the state's total
    ks = kc.isometry_kraus(rng, 3)
    rec, data = program.encode([kc.kraus_op(1, ks)])
    K, E = kraus_of_record(data, int(rec[0]["data_off"]), 3)
    u = np.linspace(0.02, 0.98, S)
    new, pick, undet = kraus_step(psi, 1, K, E, u)
    assert not undet.any()
    total = (np.abs(psi) ** 2).sum(axis=0)
    assert np.allclose((np.abs(new) ** 2).sum(axis=0), total, rtol=1e-13)
    for s in range(S):
        t = psi[:, s].reshape(2, 2, 2)                              # axes: qubit 2, 1, 0
        w = [np.linalg.norm(np.einsum("ab,ibj->iaj", k, t)) ** 2 for k in ks]
        k = int(np.searchsorted(np.cumsum(w), u[s] * total[s], side="right"))
        assert pick[s] == k
        want = np.einsum("ab,ibj->iaj", ks[k], t).ravel() * np.sqrt(total[s] / w[k])
        assert np.allclose(new[:, s], want, atol=1e-13)
    # a draw on a boundary is flagged, the top boundary included; one past the top takes the last operator with weight
    cum = np.cumsum([np.linalg.norm(np.einsum("ab,ibj->iaj", k, psi[:, 0].reshape(2, 2, 2))) ** 2 for k in ks])
    for b in cum:
        _, _, ud = kraus_step(psi[:, :1], 1, K, E, np.array([b / total[0]]))
        assert ud[0]
    _, pick, _ = kraus_step(psi[:, :1], 1, K, E, np.array([1.0 + 1e-6]))
    assert pick[0] == 2


# ---- the per-shot reference averages to the density matrix ----------------------------------------------------------------------

def _counts(words, nbits):
    vals, cnt = np.unique(words, return_counts=True)
    return {format(int(v), "0%db" % nbits): int(c) for v, c in zip(vals, cnt)}


@pytest.mark.parametrize("W, seed", [(3, 11), (5, 2 ** 40 + 3)])
def test_exact_reference_averages_to_the_density_matrix(W, seed):
    rng = np.random.RandomState(70 + W)
    rec, data = program.encode(kc.with_kraus(nc.random_ops(W, 900 + W, n_random=16), W, rng))
    assert (rec["kind"] == _lib.OP_KRAUS).sum() >= 8 and (rec["kind"] == _lib.OP_PAULI).sum() > 0
    shots = 20000
    meas = list(range(W))
    ro = np.tile([0.03, 0.06], (W, 1))
    words, alt, amb, undet = exact_kraus_sample(rec, data, W, shots, seed, meas, ro)
    assert within_cap(amb, undet)[0] <= within_cap(amb, undet)[1]
    want = kraus_density_distribution(rec, data, W, meas, ro)
    assert abs(want.sum() - 1.0) < 1e-12
    assert chi2_pvalue(_counts(words, W), want, shots) > 1e-4
    # and the shots of a call are a prefix of a larger call's
    w2 = exact_kraus_sample(rec, data, W, 50, seed, meas, ro, first_shot=100)[0]
    assert np.array_equal(w2, words[100:150])


# ---- the cap cannot hide a failure: the reference of every device case stays within it on its own -----------------------------------

@pytest.mark.parametrize("name", list(kc.GPU_CASES))
def test_reference_of_every_device_case_is_within_the_cap(name):
    words, alt, amb, undet = kc.reference(name)
    n, cap = within_cap(amb, undet)
    print("KRAUS reference case=%s shots=%d undetermined=%d ambiguous=%d cap=%d" % (name, words.size, int(undet.sum()), int(amb.sum()), cap))
    assert n <= cap
    c = kc.case(name)
    kinds = c["rec"]["kind"]
    assert (kinds == _lib.OP_KRAUS).sum() > 0
    # the reference agrees with itself through the helper (the device test does exactly this with the engine's words)
    check_kraus_words(words.copy(), words, alt, amb, undet, family="kraus self", label=name)


# ---- the comparison notices a reference made wrong the way a kernel could be --------------------------------------------------------

MUTATION_CASES = {"no_renorm": "W=3", "e_wrong_order": "W=3", "no_draw_on_m1": "W=3", "r10_conj": "W=3"}


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_comparison_fails_on_a_mutated_reference(mutation):
    name = MUTATION_CASES[mutation]
    c = kc.case(name)
    wrong = kc.reference_of(c, _mutate=mutation)[0]
    with pytest.raises(AssertionError, match="shots differ"):
        check_kraus_words(wrong, *kc.reference(name), family="kraus mutation", label=mutation)


def test_comparison_fails_on_mutations_in_the_host_path_case_too():
    """the lowered circuit under the thermal model: four-operator channels on every gate (their K^dg K are diagonal, so
    r10 has no say there)"""
    c = kc.case("lowered graph 1")
    for mutation in ("e_wrong_order", "no_renorm"):
        wrong = kc.reference_of(c, _mutate=mutation)[0]
        with pytest.raises(AssertionError, match="shots differ"):
            check_kraus_words(wrong, *kc.reference("lowered graph 1"), family="kraus mutation", label="lowered " + mutation)


def test_unknown_mutation_is_refused():
    c = kc.case("W=1")
    with pytest.raises(ValueError):
        kc.reference_of(c, _mutate="nope")


def test_too_many_undetermined_shots_fail_the_comparison():
    words, alt, amb, undet = kc.reference("W=2")
    many = undet.copy()
    many[:3] = True                                                 # cap of 2000 shots: 2
    with pytest.raises(AssertionError, match="undetermined or ambiguous"):
        check_kraus_words(words.copy(), words, alt, amb, many, family="kraus self", label="3 undetermined")
    one = undet.copy()
    one[5] = True
    bad = words.copy()
    bad[5] ^= np.uint64(1)                                          # an undetermined shot may differ ...
    check_kraus_words(bad, words, alt, amb, one, family="kraus self", label="1 undetermined")
    bad[6] ^= np.uint64(1)                                          # ... a determined one may not
    with pytest.raises(AssertionError, match="shots differ"):
        check_kraus_words(bad, words, alt, amb, one, family="kraus self", label="1 undetermined, 1 wrong")


# ---- the sign of the effect the channels exist for, on the density matrix ------------------------------------------------------------

def test_damping_raises_the_success_rate_above_its_pauli_twirl_on_the_density_matrix():
    """test_gpu_kraus.py compares two 20 000-shot success rates; each has a standard error below 0.0036, their difference
    below 0.005: the exact rates have to differ by far more than that for the comparison to mean anything"""
    from qcmrf_amd import ingest as ing_mod
    T, n = kc.success_circuit()
    rates = []
    for nm in kc.success_models(0.2):
        ing = ing_mod.ingest(T, noise=nm)
        rec, data = program.encode(ing.ops)
        meas = [ing.measure.get(c, -1) for c in range(ing.num_clbits)]
        dist = kraus_density_distribution(rec, data, ing.num_qubits, meas)
        assert abs(dist.sum() - 1.0) < 1e-12
        rates.append(kc.success_rate(dist, n))
    assert rates[0] > rates[1] + 0.05                               # ten standard errors of the measured difference
    assert kc.success_rate({"0011": 3, "1000": 1}, 2) == 0.75
