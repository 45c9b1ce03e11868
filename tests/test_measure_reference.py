"""The references of MEASURE records (tests/_measure_reference.py) on the host: the deferred-measurement identity, the
per-shot reference against the exact distribution, the comparison helper against deliberately wrong references, and the
ambiguity cap of every case the GPU tests run."""
import numpy as np
import pytest

import _kraus_cases as kc
import _measure_cases as mc
from _density_matrix import chi2_pvalue
from _kraus_reference import kraus_density_distribution, within_cap
from _measure_reference import (MUTATIONS, check_measure_words, exact_measure_sample, measure_density_distribution,
                                measure_step)
from qcmrf_amd import _lib, ir, program
from qcmrf_amd.backend import QsvBackend

_H = np.array([[1, 1], [1, -1]], dtype=np.complex128) / np.sqrt(2.0)


@pytest.fixture(scope="module")
def chain4():
    """chain(4) lowered under thermal, depolarizing and readout errors: (in place, deferred) as run() prepares them"""
    qc, nm = mc.chain_circuit(4), kc.thermal_model()
    return QsvBackend._prepare_noisy(qc, nm, "lds", "in_place"), QsvBackend._prepare_noisy(qc, nm, "lds", "deferred")


@pytest.fixture(scope="module")
def chain4_exact(chain4):
    ing, rec, data, clist, meas, readout, _, _, (mode, width, n_measure) = chain4[0]
    return measure_density_distribution(rec, data, width, meas, readout)


def test_measure_step_follows_the_contract():
    rng = np.random.RandomState(3)
    psi = rng.randn(8, 5) + 1j * rng.randn(8, 5)
    psi[:, 3] = 0.0                                                 # a state without mass
    psi[1::2, 4] = 0.0                                              # qubit 0 certainly 0
    u = np.array([0.0, 0.999999, 0.5, 0.5, 0.999999])
    for release in (0, 1):
        out, b, undet = measure_step(psi, 0, release, u)
        p0 = (np.abs(psi[0::2]) ** 2).sum(axis=0)
        tot = (np.abs(psi) ** 2).sum(axis=0)
        assert b.tolist() == [0, 1, int(not p0[2] > 0.5 * tot[2]), 0, 0] and not undet.any()
        assert np.allclose((np.abs(out) ** 2).sum(axis=0), tot)     # the mass stays
        assert not out[1::2, 0].any() and np.allclose(out[0::2, 0], psi[0::2, 0] * np.sqrt(tot[0] / p0[0]))
        kept = out[0::2, 1] if release else out[1::2, 1]
        assert not (out[1::2, 1] if release else out[0::2, 1]).any()
        assert np.allclose(kept, psi[1::2, 1] * np.sqrt(tot[1] / (tot[1] - p0[1])))
        assert np.array_equal(out[:, 3], psi[:, 3])
    assert measure_step(psi, 0, 0, p0 / np.where(tot > 0, tot, 1.0))[2].tolist() == [True, True, True, False, True]


def test_in_place_is_the_deferred_distribution(chain4, chain4_exact):
    """the deferred-measurement identity: measuring the ancillas when they occur, slots recycled, gives the distribution of
    the same circuit with every measurement at the end -- 6 qubits against 8"""
    (ing_i, _, _, _, _, _, _, _, (mode, width, n_measure)), (ing, rec, data, clist, meas, readout, _, _, info) = chain4
    assert (mode, width, ing_i.num_qubits) == ("in_place", 6, 8) and info == ("deferred", 8, 0) and n_measure > 0
    deferred = kraus_density_distribution(rec, data, 8, meas, readout)
    assert chain4_exact.shape == deferred.shape == (256,)
    assert abs(deferred.sum() - 1.0) < 1e-12
    assert np.abs(chain4_exact - deferred).max() <= 1e-12


def test_exact_reference_samples_the_exact_distribution(chain4, chain4_exact):
    ing, rec, data, clist, meas, readout, _, _, (_, width, _) = chain4[0]
    shots = 2000
    words, _, amb, undet = exact_measure_sample(rec, data, width, shots, 99, meas, readout)
    uv, uc = np.unique(words, return_counts=True)
    p = chi2_pvalue({format(int(v), "b"): int(c) for v, c in zip(uv, uc)}, chain4_exact, shots)
    print("exact_measure_sample against the exact distribution: p = %.3g" % p)
    assert p > 1e-4
    assert not undet.any()


def test_density_branches_of_a_forced_outcome():
    """X, MEASURE with release and flips (0.2, 0.3), H, final measure: bit 1 is 1 with 0.7, bit 0 uniform"""
    ops = [ir.op_x(0), mc.measure_op(0, 1, 1, (0.2, 0.3)), ir.op_u(0, _H)]
    rec, data = program.encode(ops)
    d = measure_density_distribution(rec, data, 1, [0, -1])
    assert np.allclose(d, [0.15, 0.15, 0.35, 0.35])
    rec, data = program.encode(ops[:2])
    assert np.allclose(measure_density_distribution(rec, data, 1, [0, -1]), [0.3, 0.0, 0.7, 0.0])       # the slot is back in |0>
    rec, data = program.encode([ir.op_x(0), mc.measure_op(0, 1, 0, (0.2, 0.3))])
    assert np.allclose(measure_density_distribution(rec, data, 1, [0, -1]), [0.0, 0.3, 0.0, 0.7])


@pytest.mark.parametrize("name", sorted(mc.GPU_CASES))
def test_reference_of_every_device_case_is_within_the_cap(name):
    """the cap is a condition of the word-by-word tests; a draw lands within 1e-9 of one of a MEASURE record's two
    boundaries with a chance of about 4e-9 per record and shot, so the cases hold no undetermined shot at all"""
    words, alt, amb, undet = mc.reference(name)
    n, cap = within_cap(amb, undet)
    assert words.size == mc.case(name)["shots"]
    assert n <= cap
    assert not undet.any()
    assert (mc.case(name)["rec"]["kind"] == _lib.OP_MEASURE).sum() > 0


@pytest.mark.parametrize("name", sorted(mc.RECORDED))
def test_recorded_reference_is_the_reference(name):
    """the first shots of every recorded reference, computed again"""
    c = dict(mc.case(name))
    c["shots"] = mc.RECORDED[name]
    for got, want in zip(mc.reference_of(c), mc.reference(name)):
        assert np.array_equal(got, want[:c["shots"]])


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_comparison_fails_on_a_mutated_reference(mutation):
    c = mc.case("grids")
    wrong = mc.reference_of(c, _mutate=mutation)[0]
    with pytest.raises(AssertionError, match="shots differ"):
        check_measure_words(wrong, *mc.reference("grids"), family="measure mutation", label=mutation)


def test_comparison_passes_on_the_reference_itself_and_refuses_unknown_mutations():
    ref = mc.reference("grids")
    check_measure_words(ref[0].copy(), *ref, family="measure self", label="grids")
    with pytest.raises(ValueError):
        mc.reference_of(mc.case("grids"), _mutate="nope")


def test_pauli_and_kraus_draws_do_not_depend_on_when_a_bit_is_measured(chain4):
    """stream 0 does not advance at a MEASURE record: with the measure records taken out, the program's Pauli and Kraus
    draws are the same numbers"""
    from _philox_reference import u01
    ing, rec, data, *_ = chain4[0]
    n_noise = int(np.isin(rec["kind"], (_lib.OP_PAULI, _lib.OP_KRAUS)).sum())
    assert n_noise == int(np.isin(chain4[1][1]["kind"], (_lib.OP_PAULI, _lib.OP_KRAUS)).sum())
    assert len(set(u01(5, 3, 0, np.arange(n_noise)).tolist()) & set(u01(5, 3, 3, np.arange(8)).tolist())) == 0
