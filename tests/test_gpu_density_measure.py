"""Accepted measurements taken in place on a density matrix, on the MI355X: ``qsv_density_exec_accept`` (``k_dm_measure``)
against the numpy reference of ``_density_measure_cases`` (whole vector within 1e-12), against its two-operator KRAUS twin
through ``qsv_density_exec`` on the device, closed forms, and ``run(method="density_matrix", density_measure="in_place")`` end
to end (probabilities within 1e-10).

The engine option ``density_measure_kernel`` picks the kernel of a MEASURE record: 1 ``k_dm_measure`` on every qubit, 0 the
two-operator superoperator through ``k_dm_kraus``, -1 (default) the measured rule: ``k_dm_measure`` from qubit 3 up.

First MI355X run: worst |entry - reference| 2.8e-17 with fixed bits, 2.3e-16 with every outcome forgotten, 1.5e-17
at W = 11; worst |p - reference| 2.8e-16 in place against deferred, 8.3e-17 against the Gibbs pmf of the 20-clique case, whose
accept_probability was 7.7e-15 relative off the closed form (bound 8.6e-13: 100 times the 8.6e-15 measured on the CPU between
the stand-in engine and the closed form)."""
import numpy as np
import pytest

import _density_measure_cases as dm
import _measure_cases as mc
from _density_matrix import chi2_pvalue
from qcmrf_amd import _lib, ir, program
from qcmrf_amd.backend import QsvBackend
from qcmrf_amd.qcmrf import extract_probs

pytestmark = pytest.mark.gpu

AMP_TOL, PROB_TOL = 1e-12, 1e-10


def check_vector(eng, rho, W, label):
    """whole vector, Hermiticity, trace (the reference's: it is not 1)"""
    got = eng.amplitudes()
    err = float(np.abs(got - dm.vec_of(rho)).max())
    G = got.reshape(1 << W, 1 << W).T
    herm = float(np.abs(G - G.conj().T).max())
    _, trace = eng.density_diagonal([])
    want = float(np.trace(rho).real)
    print("DENSITY MEASURE %s: W=%d max |entry - reference| = %.3g, Hermiticity %.3g, trace %.6g (reference %.6g)" % (label, W, err, herm, trace, want))
    assert err <= AMP_TOL and herm <= AMP_TOL and abs(trace - want) <= AMP_TOL
    return err


OWN, AUTO, KRAUS = 1, -1, 0                  # engine option density_measure_kernel: k_dm_measure always; from qubit 3 up; never
MIN_QUBIT = 3                                # QSV_DM_MEASURE_MIN_QUBIT


def booked(rec, W, kernel=OWN):
    """(launches, bytes) dm_channel books for a program: 32 B per amplitude for PAULI, KRAUS, KRAUS2 and for a MEASURE record
    routed through k_dm_kraus, 24 for one that k_dm_measure runs"""
    kinds = [int(k) for k in rec["kind"]]
    channels = sum(k in (_lib.OP_PAULI, _lib.OP_KRAUS, _lib.OP_KRAUS2) for k in kinds)
    ts = [int(r["qubits"][0]) for r in rec if int(r["kind"]) == _lib.OP_MEASURE]
    own = sum(kernel == OWN or (kernel == AUTO and t >= MIN_QUBIT) for t in ts)
    return channels + len(ts), (32.0 * (channels + len(ts) - own) + 24.0 * own) * 4.0 ** W


# ---- records ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", [OWN, AUTO], ids=["k_dm_measure", "auto"])
@pytest.mark.parametrize("W", dm.WIDTHS)
def test_random_program_whole_vector(W, kernel):
    """k_dm_measure on every slot (fewer blocks than lanes up to 16 workgroups), and the records as the library routes them:
    slots 0..2 through k_dm_kraus, booked at 32 B, slots 5, 6 through k_dm_measure at 24"""
    c = dm.width_case(W)
    with _lib.Engine(2 * W) as eng:
        eng.set_option("density_measure_kernel", kernel)
        eng.density_exec_accept(c["rec"], c["data"], *dm.mask_of(c["fix"]))
        check_vector(eng, c["rho"], W, "random program (%s)" % ("k_dm_measure" if kernel == OWN else "auto"))
        kq = eng.stats()["kinds"]["kq"]
        assert (kq["launches"], kq["bytes"]) == booked(c["rec"], W, kernel)
        assert W < 6 or booked(c["rec"], W, AUTO)[1] not in (booked(c["rec"], W, OWN)[1], booked(c["rec"], W, KRAUS)[1])    # both routes taken
        eng.density_exec_accept(c["rec"], c["data"], *dm.mask_of(c["fix"]))          # a second program starts from |0..0><0..0| again
        assert float(np.abs(eng.amplitudes() - dm.vec_of(c["rho"])).max()) <= AMP_TOL
        # nothing fixed: every outcome forgotten, the trace stays
        eng.density_exec_accept(c["rec"], c["data"])
        check_vector(eng, dm.reference_rho(c["rec"], c["data"], W), W, "nothing fixed")
        assert abs(eng.density_diagonal([])[1] - 1.0) <= AMP_TOL


@pytest.mark.parametrize("nt", [0, 1])
@pytest.mark.parametrize("W", dm.NT_WIDTHS)
def test_forced_nontemporal(W, nt):
    c = dm.width_case(W)
    with _lib.Engine(2 * W) as eng:
        eng.set_option("nontemporal", nt)
        eng.set_option("density_measure_kernel", OWN)
        eng.density_exec_accept(c["rec"], c["data"], *dm.mask_of(c["fix"]))
        check_vector(eng, c["rho"], W, "nontemporal=%d" % nt)


@pytest.mark.parametrize("nt", [0, 1])
def test_grid_stride_w11(nt):
    """blocks_per_cu = 1: 4^11 / 4 = 2^20 blocks on a grid of one workgroup per CU, 16 per thread on 256 CUs; both release
    forms; one QSV_K_KQ launch of 24 x 4^W bytes per MEASURE record"""
    c = dm.w11_case()
    W = c["W"]
    assert len(c["rec"]) <= 12 and np.trace(c["rho"]).real > 1e-2
    ms = c["rec"][c["rec"]["kind"] == _lib.OP_MEASURE]
    assert set(int(r) for r in ms["vals"][:, 1]) == {0, 1} and set(int(q) for q in ms["qubits"][:, 0]) == {0, 5, 10}
    with _lib.Engine(2 * W) as eng:
        eng.set_option("blocks_per_cu", 1)
        eng.set_option("nontemporal", nt)
        eng.set_option("density_measure_kernel", OWN)
        eng.reset_stats()
        eng.density_exec_accept(c["rec"], c["data"], *dm.mask_of(c["fix"]))
        kq = eng.stats()["kinds"]["kq"]
        assert (kq["launches"], kq["bytes"]) == booked(c["rec"], W)
        assert booked(ms, W) == (len(ms), 24.0 * 4.0 ** W * len(ms))
        check_vector(eng, c["rho"], W, "grid stride nontemporal=%d" % nt)


@pytest.mark.parametrize("W", dm.WIDTHS)
def test_device_cross_check_against_the_kraus_twin(W):
    """every MEASURE record as sqrt(w0) |0><0|, sqrt(w1) |1><1| (release: |0><1|) through k_dm_kraus"""
    c = dm.width_case(W)
    rec, data = dm.with_twins(c["ops"], c["fix"])
    with _lib.Engine(2 * W) as eng:
        eng.density_exec(rec, data)
        twin = eng.amplitudes()
        for kernel in (OWN, AUTO, KRAUS):
            eng.set_option("density_measure_kernel", kernel)
            eng.density_exec_accept(c["rec"], c["data"], *dm.mask_of(c["fix"]))
            err = float(np.abs(eng.amplitudes() - twin).max())
            print("DENSITY MEASURE twin: W=%d density_measure_kernel=%d max |MEASURE records - KRAUS twins| = %.3g" % (W, kernel, err))
            assert err <= AMP_TOL
            assert kernel == OWN or float(np.abs(eng.amplitudes() - dm.vec_of(c["rho"])).max()) <= AMP_TOL


@pytest.mark.parametrize("W", [3, 7])
def test_identity_without_measure_records(W):
    c = dm.width_case(W)
    rec = c["rec"][c["rec"]["kind"] != _lib.OP_MEASURE]
    with _lib.Engine(2 * W) as eng:
        eng.density_exec(rec, c["data"])
        a = eng.amplitudes()
        eng.density_exec_accept(rec, c["data"])
        b = eng.amplitudes()
        eng.density_exec_accept(rec, c["data"], 1 << 9, 1 << 9)     # a fixed bit no record writes: the caller's business
        d = eng.amplitudes()
    assert np.array_equal(a, b) and np.array_equal(a, d)


# ---- closed forms ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", [OWN, AUTO, KRAUS], ids=["k_dm_measure", "auto", "k_dm_kraus"])
@pytest.mark.parametrize("W", [1, 3, 7])
def test_closed_forms(W, kernel):
    """every other qubit in |+> (entries that are powers of two: the sums below are exact)"""
    with _lib.Engine(2 * W) as eng:
        eng.set_option("density_measure_kernel", kernel)
        for s in mc.slots(W):
            rest = [ir.op_init(((1 << W) - 1) & ~(1 << s))]
            eng.density_exec(*program.encode(rest))
            before = eng.amplitudes()
            # X, then the bit read as 1 for certain, the slot handed back: trace 1, slot in |0>, everything else as it was
            eng.density_exec_accept(*program.encode(rest + [ir.op_x(s), mc.measure_op(s, 3, 1, (0.0, 0.0))]), 1 << 3, 1 << 3)
            assert eng.density_diagonal([])[1] == 1.0
            assert eng.density_diagonal([s])[0][1] == 0.0
            assert np.array_equal(eng.amplitudes(), before), s
            # the same with the bit fixed to 0: nothing is left, exactly
            eng.density_exec_accept(*program.encode(rest + [ir.op_x(s), mc.measure_op(s, 3, 1, (0.0, 0.0))]), 1 << 3, 0)
            assert not eng.amplitudes().any()
            # flips (0.1, 0.3), X, fixed to 0: the 1 is read as 0 with probability 0.3
            for release in (0, 1):
                eng.density_exec_accept(*program.encode(rest + [ir.op_x(s), mc.measure_op(s, 63, release, (0.1, 0.3))]), 1 << 63, 0)
                assert abs(eng.density_diagonal([])[1] - 0.3) <= 1e-15
                assert abs(eng.density_diagonal([s])[0][1 - release] - 0.3) <= 1e-15


def test_refusals_leave_the_state_as_it_was():
    W = 3
    with _lib.Engine(2 * W) as eng:
        eng.density_exec(*program.encode([ir.op_x(1)]))
        before = eng.amplitudes()
        good = [ir.op_x(2), mc.measure_op(2, 5, 1, (0.1, 0.3))]

        def patched(field, value, col=None):
            rec, data = program.encode(good)
            if col is None:
                rec[field][1] = value
            else:
                rec[field][1, col] = value
            return rec, data

        for (rec, data), what in ((patched("qubits", W, 0), "qubit 3"), (patched("vals", 64, 0), "classical bit 64"),
                                  (patched("vals", 2, 1), "release flag 2"), (patched("data_off", 10 ** 6), "data range"),
                                  (patched("n", 2), "1 qubit")):
            with pytest.raises(ValueError, match="op 1.*" + what):
                eng.density_exec_accept(rec, data, 1 << 5, 0)
        for bad in (1.5, -0.1, float("nan"), float("inf")):
            rec, data = program.encode(good)
            data = np.array(data)
            data[int(rec["data_off"][1]) + 1] = bad
            with pytest.raises(ValueError, match=r"op 1.*flip probability P\(flip \| 1\)"):
                eng.density_exec_accept(rec, data, 1 << 5, 0)
        with pytest.raises(ValueError, match="bit 5"):
            eng.density_exec_accept(*program.encode(good), 1 << 4, 1 << 5)
        with pytest.raises(RuntimeError, match=r"\(-5\).*defers every measurement"):      # qsv_density_exec as it was
            eng.density_exec(*program.encode(good))
        assert np.array_equal(eng.amplitudes(), before)
        eng.density_exec_accept(*program.encode(good), 1 << 5, 0)
        assert abs(eng.density_diagonal([])[1] - 0.3) <= 1e-15


# ---- run() end to end -------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def be():
    b = QsvBackend()
    yield b
    b.close()


@pytest.mark.parametrize("which", [0, 1, 2])
def test_run_in_place_against_deferred(be, which):
    label, qc, fixed, live, full = list(dm.small_circuits())[which]
    nm = dm.small_model()
    a = be.run(qc, shots=500, seed_simulator=8, method="density_matrix", noise_model=nm, accept=fixed, density_measure="in_place").result()
    d = be.run(qc, shots=500, seed_simulator=8, method="density_matrix", noise_model=nm, accept=fixed).result()
    ma, md = a.metadata(0), d.metadata(0)
    pa, pd = dm.as_array(a.get_probabilities(), qc.num_clbits), dm.as_array(d.get_probabilities(), qc.num_clbits)
    print("DENSITY MEASURE run %s: live %d of %d qubits, max |p in place - p deferred| = %.3g, accept_probability %.15g / %.15g"
          % (label, ma["n_qubits"], md["n_qubits"], np.abs(pa - pd).max(), ma["accept_probability"], md["accept_probability"]))
    assert (ma["density_measure"], ma["n_qubits"], ma["n_circuit_qubits"], md["n_qubits"]) == ("in_place", live, full, full)
    assert np.abs(pa - pd).max() <= PROB_TOL and abs(pa.sum() - 1.0) <= 1e-12
    assert abs(ma["accept_probability"] - md["accept_probability"]) <= PROB_TOL
    assert sum(a.get_counts().values()) == 500 and set(a.get_counts()) <= set(a.get_probabilities())
    auto = be.run(qc, shots=0, method="density_matrix", noise_model=nm, accept=fixed, density_measure="auto").result()
    assert auto.metadata(0)["density_measure"] == "in_place" and auto.get_probabilities() == a.get_probabilities()


def test_run_many_cliques_exact_gibbs_and_success_probability(be):
    """6 variables on 20 cliques: 27 qubits and 26 classical bits deferred -- refused twice over --, 8 live qubits in place.
    Without the feature the in-place run is an unknown option; the deferred one is the refusal asserted below"""
    qc = mc.many_cliques()
    fixed = qc.post_selection()
    res = be.run(qc, shots=1000, seed_simulator=3, method="density_matrix", accept=fixed, density_measure="in_place").result()
    m = res.metadata(0)
    pmf, success = dm.many_cliques_closed_form()
    P, delta = extract_probs(res.get_probabilities(), 6, 21)
    rel, bound = abs(m["accept_probability"] - success) / success, dm.accept_probability_bound()
    print("DENSITY MEASURE run 6 variables, 20 cliques: W=%d, %d MEASURE records, max |p - Gibbs| = %.3g, accept_probability %.15g, "
          "closed form %.15g: relative %.3g (bound %.3g)" % (m["n_qubits"], m["n_measure_ops"], np.abs(P - pmf).max(), m["accept_probability"], success, rel, bound))
    assert (m["n_qubits"], m["n_circuit_qubits"], m["n_measure_ops"]) == (8, 27, 19)
    assert np.abs(P - pmf).max() <= PROB_TOL and abs(delta - 1.0) <= 1e-12
    assert abs(success - 9.84e-4) < 1e-6
    assert rel <= bound
    assert sum(res.get_counts().values()) == 1000 and all(k[:21] == "0" * 21 for k in res.get_counts())
    with pytest.raises(ValueError, match="at most 17 qubits"):
        be.run(qc, shots=1000, seed_simulator=3, method="density_matrix", accept=fixed, density_measure="deferred")


def test_run_many_cliques_under_the_constructed_model(be):
    qc = mc.many_cliques()
    res = be.run(qc, shots=0, method="density_matrix", accept=qc.post_selection(), density_measure="in_place",
                 noise_model=mc.constructed_model()).result()
    m = res.metadata(0)
    want, rate, _ = dm.many_cliques_stand_in("constructed")
    got, ref = dm.as_array(res.get_probabilities(), qc.num_clbits), dm.as_array(want, qc.num_clbits)
    rel, bound = abs(m["accept_probability"] - rate) / rate, dm.accept_probability_bound()
    print("DENSITY MEASURE run 6 variables, 20 cliques, constructed model: max |p - stand-in| = %.3g, accept_probability %.15g, "
          "stand-in %.15g: relative %.3g (bound %.3g); %d pauli, %d kraus records" % (np.abs(got - ref).max(), m["accept_probability"], rate, rel, bound,
                                                                                    m["n_pauli_ops"], m["n_kraus_ops"]))
    assert m["n_kraus_ops"] > 0 and m["n_measure_ops"] == 19 and rate < dm.many_cliques_closed_form()[1]
    assert np.abs(got - ref).max() <= PROB_TOL
    assert rel <= bound


def test_accepted_noisy_shots_follow_the_exact_in_place_distribution(be):
    label, qc, fixed, live, full = list(dm.small_circuits())[1]
    nm, shots = dm.small_model(), 4000
    exact = be.run(qc, shots=0, method="density_matrix", noise_model=nm, accept=fixed, density_measure="in_place").result()
    noisy = be.run(qc, shots=shots, seed_simulator=44, noise_model=nm, accept=fixed, noisy_measure="auto").result()
    assert noisy.metadata(0)["method"] == "noisy" and noisy.metadata(0)["noisy_measure"] == "in_place"
    p = chi2_pvalue(noisy.get_counts(), dm.as_array(exact.get_probabilities(), qc.num_clbits), shots)
    print("DENSITY MEASURE %s: %d accepted noisy shots against the exact in-place distribution: p = %.3g; success rate %.4f exact, %.4f estimated"
          % (label, shots, p, exact.metadata(0)["accept_probability"], noisy.metadata(0)["accept_probability"]))
    assert p > 1e-4
