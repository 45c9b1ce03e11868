"""The references of the two-qubit Kraus tests, checked on the host: the per-shot reference against the density walker,
the ambiguity cap on every GPU case, and the word comparison against deliberately wrong references."""
import numpy as np
import pytest

import _kraus2_cases as k2c
from _density_matrix import chi2_pvalue
from _kraus2_reference import (MUTATIONS, Kraus2NumpyEngine, check_kraus_words, exact_kraus2_sample, kraus2_density_distribution,
                               kraus2_of_record, within_cap)
from _noise_exact_cases import ambiguity_cap
from qcmrf_amd import _lib, program


def counts_of(words, nbits):
    out = {}
    for w in words:
        k = format(int(w), "0%db" % nbits)
        out[k] = out.get(k, 0) + 1
    return out


@pytest.mark.parametrize("W", [2, 4])
def test_trajectories_average_to_the_density_walker(W):
    """20 000 trajectories of the reference's walk (numpy random numbers) against the exact distribution"""
    rec, data = program.encode(k2c.random_ops(W, 300 + W, 16))
    assert (rec["kind"] == _lib.OP_KRAUS2).sum() >= 8
    meas = list(range(W))
    exact = kraus2_density_distribution(rec, data, W, meas)
    assert abs(exact.sum() - 1.0) < 1e-12
    words = Kraus2NumpyEngine(W).noisy_sample(rec, data, 20000, 99, meas)
    p = chi2_pvalue(counts_of(words, W), exact, 20000)
    print("KRAUS2 reference chi2 W=%d: p = %.3g" % (W, p))
    assert p > 1e-4


def test_philox_walk_averages_to_the_density_walker_too():
    c = k2c.case("W=3")
    meas = list(range(3))
    words = exact_kraus2_sample(c["rec"], c["data"], 3, 20000, 5, meas)[0]
    assert chi2_pvalue(counts_of(words, 3), kraus2_density_distribution(c["rec"], c["data"], 3, meas), 20000) > 1e-4


@pytest.mark.parametrize("name", sorted(k2c.GPU_CASES))
def test_reference_alone_stays_within_the_cap(name):
    c = k2c.case(name)
    assert c["shots"] <= 2000
    words, alt, amb, undet = k2c.reference(name)
    n, cap = within_cap(amb, undet)
    print("KRAUS2 case=%s W=%d records=%d shots=%d undetermined=%d ambiguous=%d cap=%d" % (
        name, c["W"], len(c["rec"]), c["shots"], int(undet.sum()), int(amb.sum()), cap))
    assert cap == ambiguity_cap(c["shots"]) and n <= cap
    assert (c["rec"]["kind"] == _lib.OP_KRAUS2).sum() > 0


@pytest.mark.parametrize("W", k2c.WIDTHS)
def test_width_cases_hold_what_they_promise(W):
    rec, data = k2c.case("W=%d" % W)["rec"], k2c.case("W=%d" % W)["data"]
    kinds = set(int(k) for k in rec["kind"])
    assert {_lib.OP_1Q, _lib.OP_MCX, _lib.OP_DIAG, _lib.OP_MCPHASE, _lib.OP_PAULI, _lib.OP_KRAUS, _lib.OP_KRAUS2} <= kinds
    k2 = rec[rec["kind"] == _lib.OP_KRAUS2]
    assert {1, 2, 4, 16} <= set(int(m) for m in k2["vals"][:, 0])
    assert {(int(a), int(b)) for a, b in k2["qubits"][:, :2]} == set(k2c.pairs(W))
    for r in k2:
        K, E = kraus2_of_record(data, int(r["data_off"]), int(r["vals"][0]))
        assert np.abs(np.einsum("kai,kaj->ij", K.conj(), K) - np.eye(4)).max() < 1e-12
        assert np.abs(E[:, :4].sum(axis=0) - 1.0).max() < 1e-12 and np.abs(E[:, 4:].sum(axis=0)).max() < 1e-12


def test_prefix_and_first_shot():
    c, big = k2c.case("seed"), k2c.case("prefix of 2000")
    ref, ref_big = k2c.reference("seed"), k2c.reference("prefix of 2000")
    assert all(np.array_equal(a, b[:c["shots"]]) for a, b in zip(ref, ref_big))
    tail = k2c.reference_of(dict(c, shots=100), first_shot=1400)
    assert all(np.array_equal(a, b[1400:1500]) for a, b in zip(tail, ref))
    assert big["shots"] == 2000


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_word_comparison_notices_a_wrong_reference(mutation):
    """the right words, compared against a reference made wrong the way a kernel could be, fail"""
    for name in ("W=3", "seed"):
        c = k2c.case(name)
        right = k2c.reference(name)[0]
        wrong = k2c.reference_of(c, _mutate=mutation)
        with pytest.raises(AssertionError):
            check_kraus_words(right, *wrong, family="kraus2 mutation", label="%s %s" % (mutation, name))
    check_kraus_words(right, *k2c.reference("seed"), family="kraus2 mutation", label="none")


def test_forced_programs_on_the_reference():
    for W in (3, 9):
        for label, (rec, data), want in k2c.forced_programs(W):
            words = exact_kraus2_sample(rec, data, W, 16, 23)[0]
            assert (words == want).all(), (W, label)
