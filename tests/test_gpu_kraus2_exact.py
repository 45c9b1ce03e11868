"""Two-qubit Kraus records on the MI355X, word by word: every output word of ``qsv_noisy_sample``, ``_hbm`` and ``_accept``
against the Philox-exact reference extended by the KRAUS2 contract of include/qsv.h (_kraus2_reference.py), and forced
channels against plain basis states.

Every comparison goes through ``check_kraus_words``: ``check_words`` on the shots whose Kraus draws the reference can decide.
A shot in which any Kraus draw has u * total within 1e-9 of the total of a cumulative boundary is left out, and those shots
together with the final-draw ambiguous ones may number at most max(2, shots // 1000) per case (test_kraus2_reference.py
asserts on the host that the reference of every case here stays within that cap on its own)."""
import numpy as np
import pytest

import _kraus2_cases as k2c
from _kraus2_reference import check_kraus_words
from qcmrf_amd import _lib

pytestmark = pytest.mark.gpu


def sample(eng, c, shots=None, hbm=False):
    fn = eng.noisy_sample_hbm if hbm else eng.noisy_sample
    return fn(c["rec"], c["data"], c["shots"] if shots is None else shots, c["seed"], c["meas"], c["readout"])


def run_case(name, family, hbm=False):
    c = k2c.case(name)
    with _lib.Engine(c["W"]) as eng:
        got = sample(eng, c, hbm=hbm)
    check_kraus_words(got, *k2c.reference(name), family=family, label=name + (" hbm" if hbm else ""))
    return c, got


# ---- widths: every kernel instantiation, each qubit of a pair below, at and above the lane and wave boundaries -------------------

@pytest.mark.parametrize("W", k2c.WIDTHS)
def test_random_program_with_kraus2_every_word(W):
    c = k2c.case("W=%d" % W)
    k2 = c["rec"][c["rec"]["kind"] == _lib.OP_KRAUS2]
    assert {1, 2, 4, 16} <= set(int(m) for m in k2["vals"][:, 0])
    assert {(int(a), int(b)) for a, b in k2["qubits"][:, :2]} == set(k2c.pairs(W))
    _, got = run_case("W=%d" % W, "kraus2 widths")
    assert got.max() < 2 ** W


# ---- seeds, grids, shot ranges ------------------------------------------------------------------------------------------

def test_seed_above_2_32_grids_partial_rounds_and_prefix():
    c, ref = k2c.case("seed"), k2c.reference("seed")
    assert c["seed"] > 2 ** 32
    with _lib.Engine(c["W"]) as eng:
        for grid in (1, 7):                                       # 1500 = 7 x 214 + 2: the last round of the grid is partial
            eng.set_option("noisy_grid", grid)
            check_kraus_words(sample(eng, c), *ref, family="kraus2 shot ranges", label="noisy_grid=%d" % grid)
        odd = sample(eng, c, 1237)
        check_kraus_words(odd, *(r[:1237] for r in ref), family="kraus2 shot ranges", label="1237 shots, noisy_grid=7")
        eng.set_option("noisy_grid", 0)
        full = sample(eng, c)
        big = sample(eng, k2c.case("prefix of 2000"))
    check_kraus_words(big, *k2c.reference("prefix of 2000"), family="kraus2 shot ranges", label="2000 shots")
    assert np.array_equal(big[:c["shots"]], full)                 # N shots are the first N of a larger call, bit for bit


# ---- the slot path ----------------------------------------------------------------------------------------------------------

def test_slot_path_w11_every_word():
    c, ref = k2c.case("W=11"), k2c.reference("W=11")
    with _lib.Engine(11) as eng:
        got = sample(eng, c, 256, hbm=True)
    check_kraus_words(got, *(r[:256] for r in ref), family="kraus2 slots", label="W=11, 256 shots")


def test_slot_path_w14_every_word():
    c, _ = run_case("slots W=14", "kraus2 slots", hbm=True)
    assert c["shots"] <= 256


def test_slot_path_small_width_and_grid():
    c, ref = k2c.case("seed"), k2c.reference("seed")
    with _lib.Engine(c["W"]) as eng:
        eng.set_option("noisy_grid", 7)
        check_kraus_words(sample(eng, c, hbm=True), *ref, family="kraus2 slots", label="W=4, noisy_grid=7")


# ---- qsv_noisy_sample_accept ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hbm", [False, True])
@pytest.mark.parametrize("name", ["W=8", "lowered chain(3) in_place"])
def test_accept_with_nothing_fixed_is_the_plain_call_word_for_word(name, hbm):
    c = k2c.case(name)
    shots = min(c["shots"], 400)
    with _lib.Engine(c["W"]) as eng:
        plain = sample(eng, c, shots, hbm=hbm)
        words, index, attempts = eng.noisy_sample_accept(c["rec"], c["data"], shots, c["seed"], c["meas"], c["readout"], 0, 0, hbm=hbm)
    assert attempts == shots and np.array_equal(index, np.arange(shots, dtype=np.uint64))
    assert np.array_equal(words, plain)
    check_kraus_words(words, *(r[:shots] for r in k2c.reference(name)), family="kraus2 accept", label=name)


@pytest.mark.parametrize("hbm", [False, True])
def test_accept_on_a_measured_bit_is_the_filtered_plain_run(hbm):
    c = k2c.case("lowered chain(3) in_place")
    bit = int(c["rec"][c["rec"]["kind"] == _lib.OP_MEASURE]["vals"][0, 0])     # a bit a MEASURE record writes: an ancilla
    assert c["n_measure"] > 0 and bit >= 3 and c["meas"][bit] < 0
    with _lib.Engine(c["W"]) as eng:
        words, index, attempts = eng.noisy_sample_accept(c["rec"], c["data"], 200, c["seed"], c["meas"], c["readout"], 1 << bit, 0,
                                                         hbm=hbm, max_attempts=c["shots"])
        plain = sample(eng, c, attempts, hbm=hbm)
    keep = np.flatnonzero((plain >> np.uint64(bit)) & np.uint64(1) == 0)
    assert 0 < len(words) <= 200 and attempts <= c["shots"]
    assert np.array_equal(index, keep[:len(words)].astype(np.uint64)) and np.array_equal(words, plain[keep][:len(words)])
    ref = k2c.reference("lowered chain(3) in_place")
    idx = index.astype(np.int64)
    check_kraus_words(words, *(r[idx] for r in ref), family="kraus2 accept", label="ancilla bit %d = 0" % bit)


# ---- through the host path: depolarizing + coherent two-qubit + readout errors on a chain of 3 variables ------------------------

@pytest.mark.parametrize("measure", ["deferred", "in_place"])
@pytest.mark.parametrize("shape", ["lowered", "constructed"])
def test_chain_of_3_variables_every_word(shape, measure):
    c, _ = run_case("%s chain(3) %s" % (shape, measure), "kraus2 host path")
    kinds = c["rec"]["kind"]
    assert (kinds == _lib.OP_KRAUS2).sum() > 0 and (kinds == _lib.OP_PAULI).sum() > 0
    assert ((kinds == _lib.OP_MEASURE).sum() > 0) == (measure == "in_place")
    assert c["W"] == (5 if measure == "in_place" else 6)


# ---- forced channels: plain equality, nothing of the Philox emulation involved ----------------------------------------------

@pytest.mark.parametrize("W", [3, 9, 11])
def test_forced_channels_end_in_their_state(W):
    bad = []
    with _lib.Engine(W) as eng:
        for label, (rec, data), want in k2c.forced_programs(W):
            for fn in (eng.noisy_sample, eng.noisy_sample_hbm):
                got = fn(rec, data, 64, 23)
                if not (got == want).all():
                    bad.append((label, fn.__name__, want, sorted(set(int(g) for g in got))[:4]))
    assert not bad, "program, entry point, expected state, states seen: %s" % (bad,)
