"""``qsv_noisy_sample_accept`` on the MI355X: noisy shots kept only when fixed bits of their word read given values, and
abandoned on the device as soon as a measurement taken in place contradicts.

Identity with the plain entry points, acceptance per attempt index against the Philox-exact reference (_accept_cases.py:
the rule of include/qsv.h applied to ``exact_measure_sample``) at the widths where the kernel forms change, with one and two
workgroups (abandoned and kept shots back to back in one workgroup) and in rounds of 1, 7 and the library's choice, forced
outcomes, the refusals, and ``run(accept=...)`` against the filtered plain run and the exact conditioned distribution."""
import numpy as np
import pytest

import _accept_cases as ac
import _measure_cases as mc
from _density_matrix import chi2_pvalue
from qcmrf_amd import QCMRF, _lib, get_backend, ir, program

pytestmark = pytest.mark.gpu


def plain(eng, c, shots, hbm):
    fn = eng.noisy_sample_hbm if hbm else eng.noisy_sample
    return fn(c["rec"], c["data"], shots, c["seed"], c["meas"], c["readout"])


def accept(eng, c, shots, hbm, fixed=None, **kw):
    fm, fv = ac.mask_of(fixed or {})
    return eng.noisy_sample_accept(c["rec"], c["data"], shots, c["seed"], c["meas"], c["readout"], fm, fv, hbm=hbm, **kw)


# ---- identity with the plain entry points ---------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["grids", "lds W=11"])             # W = 4 and 11: one wave and a workgroup per trajectory
@pytest.mark.parametrize("hbm", [False, True], ids=["lds", "hbm"])
def test_nothing_fixed_is_the_plain_call_word_for_word(name, hbm):
    c = mc.case(name)
    with _lib.Engine(c["W"]) as eng:
        want = plain(eng, c, 1500, hbm)
        words, index, attempts = accept(eng, c, 1500, hbm)
        assert np.array_equal(words, want) and np.array_equal(index, np.arange(1500, dtype=np.uint64)) and attempts == 1500
        # attempt t is shot t: from first_shot = 1000 on, the shots 1000.. of the longer plain call
        words, index, attempts = accept(eng, c, 500, hbm, first_shot=1000, round=64)
        assert np.array_equal(words, want[1000:]) and np.array_equal(index, np.arange(1000, 1500, dtype=np.uint64)) and attempts == 500


# ---- acceptance per attempt index against the exact reference ---------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(ac.PLANS))
def test_accepted_attempts_against_the_reference(name):
    """per attempt index, for every fixed-bit choice of the case: accepted iff the reference accepts, the same word, the same
    number of attempts; the same outputs with 1 and 2 workgroups and in rounds of 1 and 7"""
    path, choices = ac.PLANS[name]
    hbm = path == "hbm"
    for fixed in choices:
        p = ac.plan(name, fixed)
        c, window = p["case"], p["ref"][0].size
        assert window <= 2000 and p["attempts"] < window
        with _lib.Engine(c["W"]) as eng:
            first = accept(eng, c, p["shots"], hbm, fixed, max_attempts=window)
            ac.check_accept(first, p, "%s %s %r" % (name, path, fixed))
            runs = {}
            for grid in (1, 2):
                eng.set_option("noisy_grid", grid)
                runs["noisy_grid=%d" % grid] = accept(eng, c, p["shots"], hbm, fixed, max_attempts=window)
            eng.set_option("noisy_grid", 0)
            for n in (1, 7):
                runs["round=%d" % n] = accept(eng, c, p["shots"], hbm, fixed, max_attempts=window, round=n)
            eng.set_option("noisy_grid", 2)
            runs["noisy_grid=2, round=7"] = accept(eng, c, p["shots"], hbm, fixed, max_attempts=window, round=7)
        for label, got in runs.items():
            assert np.array_equal(got[0], first[0]) and np.array_equal(got[1], first[1]) and got[2] == first[2], (name, fixed, label)


def test_both_paths_accept_the_same_attempts():
    """W = 10 through the slot path too: sums in another order, no draw of this case near a boundary"""
    name, fixed = "lds W=10", ac.PLANS["lds W=10"][1][0]
    p = ac.plan(name, fixed)
    c = p["case"]
    with _lib.Engine(c["W"]) as eng:
        ac.check_accept(accept(eng, c, p["shots"], True, fixed, max_attempts=1500), p, name + " slot path")


# ---- forced outcomes --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W,hbm", [(3, False), (8, False), (11, False), (4, True), (14, True)])
def test_forced_outcomes(W, hbm):
    """all attempts accepted or none, whatever the draws: the read bit decides, only a bit's last write may end a shot,
    a bit of the final draw is filtered"""
    bad = []
    with _lib.Engine(W) as eng:
        for grid in (0, 1):
            eng.set_option("noisy_grid", grid)
            for label, (rec, data), meas, readout, fixed, every in ac.forced_accept_programs(W):
                fm, fv = ac.mask_of(fixed)
                words, index, attempts = eng.noisy_sample_accept(rec, data, 40, 17, meas, readout, fm, fv, max_attempts=200, hbm=hbm)
                if every:
                    ok = len(words) == 40 and attempts == 40 and index.tolist() == list(range(40)) and ac.accepts(words, fixed).all()
                else:
                    ok = len(words) == 0 and len(index) == 0 and attempts == 200
                if not ok:
                    bad.append((label, grid, len(words), attempts))
    assert not bad, "program, noisy_grid, accepted, attempts: %s" % (bad,)


def test_decisive_is_the_last_write_among_kept_shots():
    """a bit written twice with both outcomes open: H, MEASURE (bit 5, no release), H, MEASURE (bit 5).  Fixed to 1, half the
    attempts are accepted; a kernel that abandoned at the first write would lose the shots whose first outcome was 0"""
    h = ir.op_u(0, np.array([[1.0, 1.0], [1.0, -1.0]]) / np.sqrt(2.0))
    ops = [h, mc.measure_op(0, 5, 0, (0.0, 0.0)), h, mc.measure_op(0, 5, 0, (0.0, 0.0))]
    rec, data = program.encode(ops)
    meas = [-1] * 6
    with _lib.Engine(2) as eng:
        want = eng.noisy_sample(rec, data, 400, 3, meas)
        words, index, attempts = eng.noisy_sample_accept(rec, data, 100, 3, meas, None, 1 << 5, 1 << 5, max_attempts=400)
    keep = np.flatnonzero(want == np.uint64(1 << 5))[:100]
    assert 100 < keep[-1] < 400                                        # about half are kept
    assert np.array_equal(index, keep.astype(np.uint64)) and attempts == keep[-1] + 1 and (words == np.uint64(1 << 5)).all()


# ---- refusals ---------------------------------------------------------------------------------------------------------------

def test_refusals_name_the_bit():
    rec, data = program.encode([ir.op_x(1), mc.measure_op(1, 2, 1, (0.1, 0.2))])
    meas = [0, -1, -1, -1]
    with _lib.Engine(3) as eng:
        for hbm in (False, True):
            call = lambda fm, fv, m=meas, **kw: eng.noisy_sample_accept(rec, data, 8, 1, m, None, fm, fv, hbm=hbm, **kw)  # noqa: E731
            assert len(call(0b101, 0b100)[0]) == 8
            with pytest.raises(ValueError, match="bit 1"):
                call(0b100, 0b110)                                     # fix_val outside fix_mask
            with pytest.raises(ValueError, match="bit 4"):
                call(1 << 4, 0)                                        # at or above n_meas
            with pytest.raises(ValueError, match="bit 3"):
                call(1 << 3, 0)                                        # neither the final draw nor a MEASURE record writes it
            with pytest.raises(ValueError, match="max_attempts"):
                call(0b100, 0b100, max_attempts=0)
        plain_rec, plain_data = program.encode([ir.op_x(1)])
        with pytest.raises(ValueError, match="bit 3"):                 # full-index words: at or above the width
            eng.noisy_sample_accept(plain_rec, plain_data, 8, 1, None, None, 1 << 3, 0)
        words, _, attempts = eng.noisy_sample_accept(plain_rec, plain_data, 8, 1, None, None, 0b010, 0b010)
        assert (words == 2).all() and attempts == 8


# ---- through run() ----------------------------------------------------------------------------------------------------------

def chain3():
    qc = QCMRF(mc.chain(3), mc.chain_theta(3), with_measurements=True)
    return mc.chain_circuit(3), qc.post_selection()


def filtered(counts, fixed):
    return {k: v for k, v in counts.items() if all(k.replace(" ", "")[::-1][c] == str(b) for c, b in fixed.items())}


@pytest.mark.parametrize("measure", ["in_place", "deferred"])
@pytest.mark.parametrize("state", ["lds", "hbm"])
def test_run_accept_is_the_filtered_plain_run(measure, state):
    """the lowered 3-variable chain under thermal relaxation: the counts of ``accept`` are those of the plain run of
    ``accept_attempts`` shots with the same seed, filtered.  Fails without the feature: the option is unknown there and
    ignored, and keys with ancilla bits set appear."""
    qc, fixed = chain3()
    nm = mc.lowered_model()
    assert fixed == {4: 0, 5: 0}
    b = get_backend()
    res = b.run(qc, shots=300, seed_simulator=77, noise_model=nm, noisy_measure=measure, noisy_state=state, accept=fixed).result()
    counts, m = res.get_counts(), res.metadata()
    assert sum(counts.values()) == 300 and filtered(counts, fixed) == counts
    assert m["accept"] == fixed and (m["noisy_measure"], m["noisy_state"]) == (measure, state)
    assert 300 <= m["accept_attempts"] <= 2000
    assert m["accept_probability"] == pytest.approx(299 / (m["accept_attempts"] - 1))
    base = b.run(qc, shots=m["accept_attempts"], seed_simulator=77, noise_model=nm, noisy_measure=measure, noisy_state=state).result()
    assert filtered(base.get_counts(), fixed) == counts
    again = b.run(qc, shots=300, seed_simulator=77, noise_model=nm, noisy_measure=measure, noisy_state=state, accept=fixed,
                  accept_round=7).result()
    assert again.get_counts() == counts and again.metadata()["accept_attempts"] == m["accept_attempts"]
    b.close()


def test_run_accept_against_the_exact_conditioned_distribution():
    """counts against ``method='density_matrix', accept=...`` (chi^2, the project's bound), and the exact success probability
    inside the interval the trajectory run's attempts give for it at the same level"""
    from scipy.stats import beta
    qc, fixed = chain3()
    nm, shots = mc.lowered_model(), 400
    b = get_backend()
    res = b.run(qc, shots=shots, seed_simulator=5, noise_model=nm, noisy_measure="auto", accept=fixed).result()
    attempts = res.metadata()["accept_attempts"]
    assert attempts <= 2000 and res.metadata()["noisy_measure"] == "in_place"
    exact = b.run(qc, shots=shots, seed_simulator=5, noise_model=nm, method="density_matrix", accept=fixed).result()
    probs = exact.get_probabilities()
    assert filtered(probs, fixed) == probs and sum(probs.values()) == pytest.approx(1.0, abs=1e-12)
    dist = np.zeros(1 << len(next(iter(probs)).replace(" ", "")))
    for k, v in probs.items():
        dist[int(k.replace(" ", ""), 2)] = v
    p = chi2_pvalue(res.get_counts(), dist, shots)
    rate = exact.metadata()["accept_probability"]
    lo, hi = beta.ppf(0.5e-4, shots, attempts - shots + 1), beta.ppf(1 - 0.5e-4, shots + 1, attempts - shots)   # Clopper-Pearson
    print("accept against the exact conditioned distribution: p = %.3g; success rate %.4f exact, %d of %d attempts: [%.4f, %.4f]"
          % (p, rate, shots, attempts, lo, hi))
    assert p > 1e-4
    assert lo <= rate <= hi
    assert sum(exact.get_counts().values()) == shots and chi2_pvalue(exact.get_counts(), dist, shots) > 1e-4
    b.close()
