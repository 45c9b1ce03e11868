"""MEASURE records (QSV_OP_MEASURE: a mid-circuit measurement taken in place, the qubit handed back) on the MI355X, word
by word: every output word of ``qsv_noisy_sample`` and ``qsv_noisy_sample_hbm`` against the Philox-exact reference
extended by the contract of include/qsv.h (_measure_reference.py), forced outcomes against plain words, the refusals,
and ``run(noisy_measure="in_place")`` against the exact distribution and on the circuit only this mode reaches.

Every word comparison goes through ``check_measure_words`` (``check_kraus_words``: undetermined and ambiguous shots at most
max(2, shots // 1000) per case; test_measure_reference.py asserts on the host that the cases hold none undetermined)."""
import numpy as np
import pytest

import _kraus_cases as kc
import _measure_cases as mc
from _density_matrix import chi2_pvalue
from _measure_reference import check_measure_words
from oracle import closed_form
from qcmrf_amd import _lib, get_backend, ir, program

pytestmark = pytest.mark.gpu


def sample(eng, c, shots=None, hbm=False):
    fn = eng.noisy_sample_hbm if hbm else eng.noisy_sample
    return fn(c["rec"], c["data"], c["shots"] if shots is None else shots, c["seed"], c["meas"], c["readout"])


def check_case_records(c, W):
    rec = c["rec"]
    kinds = set(int(k) for k in rec["kind"])
    want = {_lib.OP_1Q, _lib.OP_MCX, _lib.OP_DIAG, _lib.OP_MCPHASE, _lib.OP_PAULI, _lib.OP_KRAUS, _lib.OP_MEASURE}
    assert want <= kinds
    m = rec[rec["kind"] == _lib.OP_MEASURE]
    assert set(int(q) for q in m["qubits"][:, 0]) == set(mc.slots(W))
    assert set(int(b) for b in m["vals"][:, 0]) == set(mc.CLBITS) and set(int(r) for r in m["vals"][:, 1]) == {0, 1}
    flips = {tuple(c["data"][int(o):int(o) + 2]) for o in m["data_off"]}
    assert (0.0, 0.0) in flips and (1.0, 1.0) in flips and any(0.0 < f[0] < 1.0 for f in flips)
    last = int(np.flatnonzero((rec["kind"] == _lib.OP_MEASURE) & (rec["vals"][:, 1] == 1))[0])
    assert np.isin(rec["kind"][last + 1:], (_lib.OP_1Q, _lib.OP_MCX, _lib.OP_DIAG, _lib.OP_MCPHASE)).any()   # a released slot is used again


# ---- widths, LDS path -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W", mc.WIDTHS)
def test_random_program_with_measures_every_word(W):
    name = "lds W=%d" % W
    c = mc.case(name)
    assert c["shots"] == 1500
    check_case_records(c, W)
    with _lib.Engine(W) as eng:
        got = sample(eng, c)
    check_measure_words(got, *mc.reference(name), family="measure widths", label=name)


# ---- widths, slot path --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W", mc.HBM_WIDTHS)
def test_slot_path_same_cases_every_word(W):
    name = "lds W=%d" % W
    c = mc.case(name)
    with _lib.Engine(W) as eng:
        got = sample(eng, c, hbm=True)
    check_measure_words(got, *mc.reference(name), family="measure slot path", label=name)


@pytest.mark.parametrize("W", mc.WIDE_WIDTHS)
def test_slot_path_wide_every_word(W):
    name = "wide W=%d" % W
    c = mc.case(name)
    assert c["shots"] == mc.WIDE_SHOTS[W]
    check_case_records(c, W)
    with _lib.Engine(W) as eng:
        got = sample(eng, c, hbm=True)
    check_measure_words(got, *mc.reference(name), family="measure slot path", label=name)


# ---- grids, partial rounds, prefixes ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("hbm", [False, True], ids=["lds", "hbm"])
def test_grids_partial_rounds_and_prefix(hbm):
    c, ref = mc.case("grids"), mc.reference("grids")
    with _lib.Engine(c["W"]) as eng:
        for grid in (1, 7):                                       # 1500 = 7 x 214 + 2: the last round of the grid is partial
            eng.set_option("noisy_grid", grid)
            check_measure_words(sample(eng, c, hbm=hbm), *ref, family="measure shot ranges", label="noisy_grid=%d" % grid)
        odd = sample(eng, c, 1237, hbm=hbm)
        check_measure_words(odd, *(r[:1237] for r in ref), family="measure shot ranges", label="1237 shots, noisy_grid=7")
        eng.set_option("noisy_grid", 0)
        full = sample(eng, c, hbm=hbm)
        big = sample(eng, mc.case("prefix of 4000"), hbm=hbm)
    check_measure_words(big, *mc.reference("prefix of 4000"), family="measure shot ranges", label="4000 shots")
    assert np.array_equal(big[:c["shots"]], full)                 # N shots are the first N of a larger call, bit for bit


# ---- forced outcomes: plain equality ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W,hbm", [(4, False), (11, False), (14, True)])
def test_forced_outcomes(W, hbm):
    bad = []
    with _lib.Engine(W) as eng:
        fn = eng.noisy_sample_hbm if hbm else eng.noisy_sample
        for label, (rec, data), meas, want in mc.forced_programs(W):
            got = fn(rec, data, 64, 23, meas)
            if not (got == np.uint64(want)).all():
                bad.append((label, hex(want), sorted(set(hex(int(g)) for g in got))[:4]))
    assert not bad, "program, expected word, words seen: %s" % (bad,)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------

def test_refusals():
    ok = mc.measure_op(1, 2, 1, (0.1, 0.2))
    rec, data = program.encode([ir.op_x(1), ok])
    with _lib.Engine(3) as eng:
        assert eng.noisy_sample(rec, data, 8, 1, [-1, -1, -1]).tolist() == eng.noisy_sample_hbm(rec, data, 8, 1, [-1, -1, -1]).tolist()
        for fn in (eng.noisy_sample, eng.noisy_sample_hbm):
            with pytest.raises(ValueError, match="MEASURE"):
                fn(rec, data, 8, 1)                                   # full-index words have no classical bits
            with pytest.raises(ValueError, match="MEASURE"):
                fn(rec, data, 8, 1, [-1, -1])                         # c >= n_meas
            with pytest.raises(ValueError, match="MEASURE"):
                fn(rec, data, 8, 1, [-1, -1, 0])                      # the final draw writes the bit too
            bad = data.copy()
            bad[int(rec[1]["data_off"])] = 1.5
            with pytest.raises(ValueError, match="MEASURE"):
                fn(rec, bad, 8, 1, [-1, -1, -1])
            wide = rec.copy()
            wide[1]["qubits"][0] = 3
            with pytest.raises(ValueError, match="MEASURE"):
                fn(wide, data, 8, 1, [-1, -1, -1])
        with pytest.raises(ValueError, match="MEASURE"):
            eng.exec(rec, data)
    with _lib.Engine(6) as eng:
        with pytest.raises(RuntimeError, match="MEASURE"):             # QSV_E_UNSUPPORTED, as for the kinds it has no exact form of
            eng.density_exec(rec, data)


# ---- through run() ------------------------------------------------------------------------------------------------------------

def test_run_in_place_against_the_exact_distribution():
    """chain(4) lowered under thermal, depolarizing and readout errors: 20 000 shots at 6 live qubits against the exact
    distribution of the same circuit and model, deferred, 8 qubits (method='density_matrix'); the noise is far outside
    the sampling error: against the ideal closed form the same counts give p < 1e-12"""
    qc, nm, shots = mc.chain_circuit(4), kc.thermal_model(), 20000
    b = get_backend()
    res = b.run(qc, shots=shots, seed_simulator=31, noise_model=nm, noisy_measure="in_place").result()
    m = res.metadata()
    assert (m["noisy_measure"], m["n_qubits"], m["n_circuit_qubits"], m["noisy_state"]) == ("in_place", 6, 8, "lds")
    exact = b.run(qc, shots=1, seed_simulator=1, noise_model=nm, method="density_matrix").result()
    assert exact.metadata()["n_qubits"] == 8
    dist = np.zeros(256)
    for k, v in exact.get_probabilities().items():
        dist[int(k.replace(" ", ""), 2)] = v
    p = chi2_pvalue(res.get_counts(), dist, shots)
    flat = closed_form.probabilities(mc.chain(4), mc.chain_theta(4))              # the ideal closed form over the 8-bit words
    p_ideal = chi2_pvalue(res.get_counts(), flat, shots)
    print("in place against the exact noisy distribution: p = %.3g; against the ideal one: p = %.3g" % (p, p_ideal))
    assert p > 1e-4
    assert p_ideal < 1e-12
    b.close()


def test_run_many_cliques_only_in_place_every_word():
    """6 variables on 20 cliques: 27 qubits deferred, refused in every noisy_state; 8 live qubits in place"""
    qc, nm = mc.many_cliques(), mc.constructed_model()
    name = "6 variables, 20 cliques"
    c = mc.case(name)
    b = get_backend()
    for state in ("lds", "hbm", "auto"):
        with pytest.raises(ValueError):
            b.run(qc, shots=c["shots"], seed_simulator=c["seed"], noise_model=nm, noisy_state=state)
    res = b.run(qc, shots=c["shots"], seed_simulator=c["seed"], noise_model=nm, noisy_measure="in_place").result()
    assert res.metadata()["n_qubits"] == 8 and res.metadata()["n_measure_ops"] == c["n_measure"] == 19
    words, alt, amb, undet = mc.reference(name)
    check_counts_are_words(res.get_counts(), words, alt, amb, undet, name)
    with _lib.Engine(8) as eng:
        check_measure_words(sample(eng, c), words, alt, amb, undet, family="measure host path", label=name)
    b.close()


def test_run_slot_path_chain12_every_word():
    """chain(12) constructed: 14 live qubits, noisy_state='auto' resolves to the slot path"""
    qc, nm = mc.chain_circuit(12, lowered=False), mc.constructed_model()
    name = "chain(12)"
    c = mc.case(name)
    assert c["W"] == 14 and c["state"] == "hbm" and c["shots"] == 256
    b = get_backend()
    res = b.run(qc, shots=c["shots"], seed_simulator=c["seed"], noise_model=nm, noisy_measure="in_place", noisy_state="auto").result()
    m = res.metadata()
    assert (m["n_qubits"], m["n_circuit_qubits"], m["noisy_state"], m["noisy_measure"]) == (14, 24, "hbm", "in_place")
    words, alt, amb, undet = mc.reference(name)
    check_counts_are_words(res.get_counts(), words, alt, amb, undet, name)
    with _lib.Engine(14) as eng:
        check_measure_words(sample(eng, c, hbm=True), words, alt, amb, undet, family="measure host path", label=name)
    b.close()


def check_counts_are_words(counts, words, alt, amb, undet, name):
    """run() returns counts, not words: with no ambiguous and no undetermined shot in the case the counts are exactly the
    histogram of the reference's words (the engine call underneath is then compared word by word as well)"""
    assert not amb.any() and not undet.any(), "%s: the case was chosen to hold no ambiguous shot" % name
    uv, uc = np.unique(words, return_counts=True)
    got = {int(k.replace(" ", ""), 2): v for k, v in counts.items()}
    assert got == {int(v): int(n) for v, n in zip(uv, uc)}
