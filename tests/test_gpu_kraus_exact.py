"""Kraus records on the MI355X, word by word: every output word of ``qsv_noisy_sample`` against the Philox-exact
reference extended by the Kraus contract of include/qsv.h (_kraus_reference.py), and forced channels against plain
basis states.

Every comparison goes through ``check_kraus_words``: ``check_words`` on the shots whose Kraus draws the reference can
decide.  A shot in which any Kraus draw has u * total within 1e-9 of the total of a cumulative boundary is left out, and
those shots together with the final-draw ambiguous ones may number at most max(2, shots // 1000) per case
(test_kraus_reference.py asserts on the host that the reference of every case here stays within that cap on its own)."""
import numpy as np
import pytest

import _kraus_cases as kc
from _kraus_reference import check_kraus_words
from qcmrf_amd import _lib

pytestmark = pytest.mark.gpu


def sample(eng, c, shots=None):
    return eng.noisy_sample(c["rec"], c["data"], c["shots"] if shots is None else shots, c["seed"], c["meas"], c["readout"])


def run_case(name, family):
    c = kc.case(name)
    with _lib.Engine(c["W"]) as eng:
        got = sample(eng, c)
    check_kraus_words(got, *kc.reference(name), family=family, label=name)
    return c, got


# ---- widths: both thread counts, fewer amplitudes than lanes, the full LDS; Kraus targets 0, 5, 6, 7, 8, W - 1 ----------

@pytest.mark.parametrize("W", kc.WIDTHS)
def test_random_program_with_kraus_every_word(W):
    c = kc.case("W=%d" % W)
    rec = c["rec"]
    kinds = set(int(k) for k in rec["kind"])
    assert {_lib.OP_1Q, _lib.OP_MCX, _lib.OP_DIAG, _lib.OP_MCPHASE, _lib.OP_PAULI, _lib.OP_KRAUS} <= kinds
    kr = rec[rec["kind"] == _lib.OP_KRAUS]
    assert set(int(m) for m in kr["vals"][:, 0]) == {1, 2, 3, 4}
    assert set(int(q) for q in kr["qubits"][:, 0]) == set(kc.targets(W))
    _, got = run_case("W=%d" % W, "kraus widths")
    assert got.max() < 2 ** W


def test_realistic_parameters_every_word():
    run_case("realistic 1e-3", "kraus realistic")


# ---- seeds, grids, shot ranges ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", kc.BIG_SEEDS)
def test_seeds_above_2_32(seed):
    run_case("seed %#x" % seed, "kraus seeds")


def test_grids_partial_rounds_and_prefix():
    name = "seed %#x" % kc.BIG_SEEDS[0]
    c, ref = kc.case(name), kc.reference(name)
    with _lib.Engine(c["W"]) as eng:
        for grid in (1, 7):                                       # 1500 = 7 x 214 + 2: the last round of the grid is partial
            eng.set_option("noisy_grid", grid)
            check_kraus_words(sample(eng, c), *ref, family="kraus shot ranges", label="noisy_grid=%d" % grid)
        odd = sample(eng, c, 1237)
        check_kraus_words(odd, *(r[:1237] for r in ref), family="kraus shot ranges", label="1237 shots, noisy_grid=7")
        eng.set_option("noisy_grid", 0)
        full = sample(eng, c)
        big_case = kc.case("prefix of 6000")
        big = sample(eng, big_case)
    check_kraus_words(big, *kc.reference("prefix of 6000"), family="kraus shot ranges", label="6000 shots")
    assert np.array_equal(big[:c["shots"]], full)                 # N shots are the first N of a larger call, bit for bit


# ---- through the host path ------------------------------------------------------------------------------------------------

def test_lowered_reference_graph_thermal_model_every_word():
    c, _ = run_case("lowered graph 1", "kraus host path")
    kinds = c["rec"]["kind"]
    assert (kinds == _lib.OP_KRAUS).sum() > 0 and (kinds == _lib.OP_PAULI).sum() > 0 and c["readout"] is not None


def test_constructed_circuit_thermal_model_every_word():
    c, _ = run_case("constructed graph 2", "kraus host path")
    assert (c["rec"]["kind"] == _lib.OP_KRAUS).sum() > 0


# ---- forced channels: plain equality, nothing of the Philox emulation involved ------------------------------------------------

@pytest.mark.parametrize("W", [4, 11])
def test_forced_channels_end_in_their_state(W):
    bad = []
    with _lib.Engine(W) as eng:
        for label, (rec, data), want in kc.forced_programs(W):
            got = eng.noisy_sample(rec, data, 64, 23)
            if not (got == want).all():
                bad.append((label, want, sorted(set(int(g) for g in got))[:4]))
    assert not bad, "program, expected state, states seen: %s" % (bad,)
