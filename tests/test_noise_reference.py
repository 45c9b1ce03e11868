"""The Philox-exact reference of noisy shots (_philox_reference.py) is checked here before it judges the kernel
(test_gpu_noise_exact.py): Random123's known answers, the documented (seed, shot, stream, draw) convention, its counts
against the density matrix, and the teeth of the comparison helper.  No GPU needed."""
import numpy as np
import pytest

import _noise_exact_cases as nc
from _density_matrix import chi2_pvalue, density_distribution
from _philox_reference import MUTATIONS, TOL, exact_noisy_sample, philox4x32_10, pick_basis_state, record_words, u01, words_to_u01
from oracle import closed_form as cf
from qcmrf_amd import QCMRF, ingest as ing_mod, program
from qcmrf_amd.noise import NoiseModel, depolarizing_error
from qcmrf_amd.transpile import transpile


# ---- the generator ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("counter, key, want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(counter, key, want):
    """the three philox4x32-10 vectors of Random123's kat_vectors"""
    assert tuple(int(x) for x in philox4x32_10(counter, key)) == want


def test_philox_is_vectorised_over_any_word():
    c2 = np.array([0, 0xffffffff, 0x13198a2e], dtype=np.uint64)
    out = philox4x32_10((np.array([0, 0xffffffff, 0x243f6a88]), np.array([0, 0xffffffff, 0x85a308d3]), c2,
                         np.array([0, 0xffffffff, 0x03707344])),
                        (np.array([0, 0xffffffff, 0xa4093822]), np.array([0, 0xffffffff, 0x299f31d0])))
    assert out.shape == (3, 4) and out.dtype == np.uint32
    assert [hex(x) for x in out[:, 0]] == ["0x6627e8d5", "0x408f276d", "0xd16cfe09"]


def test_u01_range_granularity_and_word_order():
    assert words_to_u01(0xffffffff, 0xffffffff) == 1.0 - 2.0 ** -53          # the largest value is below 1
    assert words_to_u01(0, 0x7ff) == 0.0                                     # the low 11 bits are dropped
    assert words_to_u01(0, 0x800) == 2.0 ** -53
    assert words_to_u01(0x80000000, 0) == 0.5                                # c0 is the high word
    u = u01(1984, np.arange(20000), 1, 0)
    assert u.dtype == np.float64 and (u >= 0).all() and (u < 1).all()
    scaled = u * 2.0 ** 53
    assert (scaled == np.floor(scaled)).all()
    assert (scaled % 2 == 1).any()                                           # the 53rd bit is in use
    assert abs(u.mean() - 0.5) < 0.01
    # counter = (draw, stream, shot lo, shot hi), key = (seed lo, seed hi)
    seed, shot = 0x299f31d0a4093822, 0x0370734413198a2e
    assert u01(seed, shot, 0x85a308d3, 0x243f6a88) == words_to_u01(0xd16cfe09, 0x94fdcceb)


def test_u01_every_coordinate_matters():
    base = dict(seed=5, shot=9, stream=0, draw=3)
    variants = [base, dict(base, stream=1), dict(base, stream=2), dict(base, draw=4), dict(base, shot=10),
                dict(base, seed=6),
                dict(base, seed=5 + 2 ** 32),                 # only the high seed word
                dict(base, shot=9 + 2 ** 32),                 # only the high shot word
                dict(base, stream=3, draw=0), dict(base, stream=0, draw=0), dict(base, seed=2 ** 64 - 1), dict(base, seed=2 ** 63 + 5)]
    vals = [float(u01(v["seed"], v["shot"], v["stream"], v["draw"])) for v in variants]
    assert len(set(vals)) == len(vals)
    grid = u01(np.uint64(77), np.arange(64, dtype=np.uint64)[:, None], 2, np.arange(64)[None, :])
    assert np.unique(grid).size == 64 * 64


# ---- the pieces of a shot ----------------------------------------------------------------------------------------------

def test_pick_basis_state_boundaries_and_ambiguity():
    prob = np.array([0.25, 0.0, 0.5, 0.0, 0.25, 0.0])
    u = np.array([0.0, 0.2, 0.25, 0.25 - 1e-10, 0.25 + 1e-10, 0.5, 0.75 - 1e-12, 0.99, 1.0 - 2.0 ** -53, 0.25 + 1e-8])
    k, alt, amb = pick_basis_state(np.repeat(prob[:, None], u.size, axis=1), u)
    assert k.tolist() == [0, 0, 2, 0, 2, 2, 2, 4, 4, 2]
    assert amb.tolist() == [False, False, True, True, True, False, True, False, False, False]
    assert alt.tolist() == [0, 0, 0, 2, 0, 2, 4, 4, 4, 2]                    # the neighbour with mass, never index 1 or 3
    # the same picture whatever the total mass: the draw is scaled by it
    k2, alt2, amb2 = pick_basis_state(np.repeat(3.0 * prob[:, None], u.size, axis=1), u)
    assert k2.tolist() == k.tolist() and amb2.tolist() == amb.tolist()
    # rounding slack: no cumulative sum exceeds the draw -> the last index with mass; no mass at all -> 0
    tiny = np.array([[1.0], [2.0 ** -60], [0.0]])
    assert pick_basis_state(tiny, np.array([1.0 - 2.0 ** -53]))[0].tolist() == [0]
    assert pick_basis_state(np.array([[0.5], [0.5], [0.0]]), np.array([1.0]))[0].tolist() == [1]
    assert pick_basis_state(np.zeros((4, 1)), np.array([0.3]))[0].tolist() == [0]
    assert TOL == 1e-9


def test_record_words_mapping_and_flips():
    idx = np.array([0b101, 0b010], dtype=np.uint64)
    shot = np.arange(2, dtype=np.uint64)
    assert record_words(idx, 1, shot, None, None).tolist() == [5, 2]
    assert record_words(idx, 1, shot, [], None).tolist() == [0, 0]
    assert record_words(idx, 1, shot, [2, -1, 0, 0, 1], None).tolist() == [0b01101, 0b10000]
    sure = [[1.0, 0.0], [1.0, 1.0], [0.0, 1.0]]                             # a 0 in bit 0 flips, a 1 does not; bit 1 is unmeasured; a 1 in bit 2 flips, a 0 does not
    assert record_words(idx, 1, shot, [1, -1, 0], sure).tolist() == [0b001, 0b001]
    ro = [[0.5, 0.5]] * 3
    flips = np.array([[float(u01(9, s, 2, j)) < 0.5 for j in range(3)] for s in range(2)])
    got = record_words(idx, 9, shot, [0, 1, 2], ro)
    want = [int(idx[s]) ^ sum(int(flips[s, j]) << j for j in range(3)) for s in range(2)]
    assert got.tolist() == want


# ---- whole calls ---------------------------------------------------------------------------------------------------------

def counts_of(words, nb):
    vals, n = np.unique(words, return_counts=True)
    return {format(int(v), "0%db" % nb): int(c) for v, c in zip(vals, n)}


def chi2_of_case(case, shots):
    words, _, amb = exact_noisy_sample(case["rec"], case["data"], case["W"], shots, case["seed"], case["meas"], case["readout"])
    want = density_distribution(case["rec"], case["data"], case["W"], case["meas"], case["readout"])
    assert amb.sum() <= nc.ambiguity_cap(shots)
    return chi2_pvalue(counts_of(words, len(case["meas"])), want, shots), counts_of(words, len(case["meas"]))


def test_counts_follow_the_density_matrix_lowered_graph():
    case = nc.lowered_case(1)                                     # W = 4, 572 records, readout errors
    assert case["W"] <= 6 and case["readout"] is not None
    p, counts = chi2_of_case(case, 20000)
    assert p > 1e-4
    g = nc.models_05()
    assert chi2_pvalue(counts, cf.probabilities(g["GRAPHS"][1], g["THETAS"]["1"][1]), 20000) < 1e-12


def test_counts_follow_the_density_matrix_constructed_graph():
    g = nc.models_05()
    qc = QCMRF(g["GRAPHS"][1], g["THETAS"]["1"][1], with_measurements=True)
    nm = nc.reference_model()
    nm.add_all_qubit_quantum_error(depolarizing_error(0.02, 1), "h")
    case = nc.ingested_case(qc, nm, 321)
    assert case["W"] <= 6 and (case["rec"]["kind"] == 9).sum() > 0
    assert chi2_of_case(case, 20000)[0] > 1e-4


def test_zero_probability_errors_follow_closed_form():
    g = nc.models_05()
    C, th = g["GRAPHS"][1], g["THETAS"]["1"][2]
    zero = NoiseModel()
    zero.add_all_qubit_quantum_error(depolarizing_error(0.0, 1), ["sx", "x"])
    zero.add_all_qubit_quantum_error(depolarizing_error(0.0, 2), ["cx"])
    ing = ing_mod.ingest(transpile(QCMRF(C, th, with_measurements=True), basis_gates=nc.BASIS), noise=zero)
    assert ing.n_pauli > 0
    rec, data = program.encode(ing.ops)
    meas = [ing.measure.get(c, -1) for c in range(ing.num_clbits)]
    words, _, _ = exact_noisy_sample(rec, data, ing.num_qubits, 20000, 5, meas)
    assert chi2_pvalue(counts_of(words, len(meas)), cf.probabilities(C, th), 20000) > 1e-4


def test_first_shot_is_a_slice_of_the_larger_call():
    case = nc.seed_case(2 ** 63 + 12345)
    args = (case["rec"], case["data"], case["W"], )
    tail = (case["seed"], case["meas"], case["readout"])
    big = exact_noisy_sample(*args, 900, *tail)
    part = exact_noisy_sample(*args, 300, *tail, first_shot=450)
    for a, b in zip(big, part):
        assert np.array_equal(a[450:750], b)
    blocks = exact_noisy_sample(*args, 900, *tail, block=16 * 64)               # the internal blocking changes nothing
    assert np.array_equal(blocks[0], big[0])
    high = exact_noisy_sample(*args, 50, *tail, first_shot=2 ** 32)            # the high shot word reaches the counter
    assert not np.array_equal(high[0], big[0][:50])


# ---- the helper has teeth: a reference made wrong the way a kernel could be is caught ----------------------------------------

def _caught(case, mutation):
    good = nc.reference_of(case)
    bad = nc.reference_of(case, _mutate=mutation)[0]
    try:
        nc.check_words(bad, *good, family="mutation", label=mutation)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_helper_catches_a_wrong_reference(mutation):
    cases = {"width 3": nc.width_case(3), "width 6": nc.width_case(6), "lowered graph 1": nc.lowered_case(1),
             "identity-heavy": nc.identity_heavy_case(), "seed 2^32": nc.seed_case(2 ** 32), "seed 2^32 - 1": nc.seed_case(2 ** 32 - 1)}
    caught = {name: _caught(c, mutation) for name, c in cases.items()}
    print("MUTATION %s caught by %d of %d: %s" % (mutation, sum(caught.values()), len(caught), caught))
    if mutation == "seed_lo_only":
        assert caught["seed 2^32"] and not caught["seed 2^32 - 1"]      # a seed below 2^32 cannot tell
    elif mutation == "no_draw_on_identity":
        assert caught["identity-heavy"] and caught["lowered graph 1"]
    else:
        assert caught["width 3"] and caught["width 6"] and caught["lowered graph 1"]
    good = nc.reference_of(cases["width 3"])
    nc.check_words(good[0], *good, family="mutation", label="unchanged")     # and the true words pass


def test_forced_pauli_programs_end_in_one_basis_state():
    """the expectation of the forced-Pauli GPU cases (x mask, z mask) against the reference, which does not share it"""
    W = 4
    for qubits, p in nc.forced_pauli_cases(W):
        for (rec, data), want in nc.forced_pauli_programs(W, qubits, p):
            words, _, amb = exact_noisy_sample(rec, data, W, 8, 3)
            assert not amb.any() and (words == want).all(), (qubits, p)
    # swapping the x and z bits of error qubit 1 changes the end state of some forced two-qubit Pauli
    (rec, data), want = nc.forced_pauli_programs(W, (0, 3), 4)[0]
    assert (exact_noisy_sample(rec, data, W, 8, 3, _mutate="swap_xz_q1")[0] != want).all()


def test_width_cases_hold_the_mix_they_promise():
    from qcmrf_amd import _lib
    diag_n, ctrl_n, inits = set(), set(), set()
    for W in nc.WIDTHS:
        rec = nc.width_case(W)["rec"]
        kind, n = rec["kind"], rec["n"]
        diag_n |= set(n[kind == _lib.OP_DIAG].tolist())
        gates = rec[(kind == _lib.OP_1Q) | (kind == _lib.OP_MCX)]
        ctrl_n |= set(gates["n"].tolist())
        assert {0, W - 1} <= set(gates["target"].tolist())
        if W >= 2:
            assert any(0 in r["vals"][:r["n"]] and 1 in r["vals"][:r["n"]] for r in gates if r["n"] >= 2) or W == 2
            pairs = [tuple(r["qubits"][:2]) for r in rec[(kind == _lib.OP_PAULI) & (n == 2)]]
            assert any(a < b for a, b in pairs) and any(a > b for a, b in pairs)
            assert (0, W - 1) in pairs and (W - 1, 0) in pairs
        assert ((kind == _lib.OP_PAULI) & (n == 1)).any() and (kind == _lib.OP_MCPHASE).any()
        where = np.flatnonzero((kind == _lib.OP_INIT_UNIFORM) | (kind == _lib.OP_INIT_ZERO))
        inits.add(nc.WIDTH_INIT[W])
        assert {"uniform": where.tolist() == [0] and kind[0] == _lib.OP_INIT_UNIFORM, "zero": where.tolist() == [0] and kind[0] == _lib.OP_INIT_ZERO,
                "mid": where.size == 1 and where[0] > 10 and kind[where[0]] == _lib.OP_INIT_UNIFORM, None: where.size == 0}[nc.WIDTH_INIT[W]]
        if kind[where].tolist() == [_lib.OP_INIT_UNIFORM]:
            mask = int(rec["mask"][where[0]])
            assert 0 < mask < (1 << W) - 1 or W == 1                          # a partial mask
    assert {1, 8} <= diag_n and ctrl_n == {0, 1, 2, 3, 4} and inits == {"uniform", "mid", "zero", None}
