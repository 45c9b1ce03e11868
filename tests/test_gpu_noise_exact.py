"""Noisy shots on the MI355X, word by word: every output word of a ``qsv_noisy_sample`` call against the Philox-exact
trajectory reference (_philox_reference.py), and forced Paulis against plain basis states.  The counts of
test_gpu_noise.py cannot see an error that moves a fraction of a percent of the mass or that repeats on every run;
one wrong shot fails here.

Every comparison goes through ``check_words``: equal words where the reference is sure, one of two candidates where the
final draw lies within 1e-9 of the total mass of a cumulative boundary (at most max(2, shots // 1000) such shots)."""
import numpy as np
import pytest

import _noise_exact_cases as nc
from _noise_exact_cases import check_words
from _philox_reference import exact_noisy_sample
from qcmrf_amd import _lib, program

pytestmark = pytest.mark.gpu


def run_case(case, family, label, eng=None):
    """the engine's words of a case against the reference's"""
    ref = nc.reference_of(case)
    if eng is None:
        with _lib.Engine(case["W"]) as e:
            got = e.noisy_sample(case["rec"], case["data"], case["shots"], case["seed"], case["meas"], case["readout"])
    else:
        got = eng.noisy_sample(case["rec"], case["data"], case["shots"], case["seed"], case["meas"], case["readout"])
    check_words(got, *ref, family=family, label=label)
    return got


# ---- widths: both thread counts, fewer amplitudes than sampling lanes, every record kind ------------------------------------

@pytest.mark.parametrize("W", nc.WIDTHS)
def test_random_program_every_word(W):
    case = nc.width_case(W)
    kinds = set(int(k) for k in case["rec"]["kind"])
    assert {_lib.OP_1Q, _lib.OP_MCX, _lib.OP_DIAG, _lib.OP_MCPHASE, _lib.OP_PAULI} <= kinds
    assert 40 <= len(case["rec"]) <= 90
    got = run_case(case, "widths", "W=%d init=%s" % (W, nc.WIDTH_INIT[W]))
    assert got.max() < 2 ** W


# ---- forced Paulis: plain equality, nothing of the Philox emulation involved ---------------------------------------------------

@pytest.mark.parametrize("W", [4, 11])
def test_forced_paulis_end_in_their_mask(W):
    shots, n, bad = 64, 0, []
    with _lib.Engine(W) as eng:
        for qubits, p in nc.forced_pauli_cases(W):
            for which, ((rec, data), want) in zip(("P|0>", "H P H|0>"), nc.forced_pauli_programs(W, qubits, p)):
                got = eng.noisy_sample(rec, data, shots, 17 + p)
                n += shots
                if not (got == want).all():
                    bad.append((which, qubits, p, want, sorted(set(int(g) for g in got))[:4]))
    t = nc.TALLY.setdefault("forced", [0, 0, 0])
    t[0] += n
    t[2] += len(bad)
    print("EXACT family=forced case=W=%d shots=%d ambiguous=0 mismatching programs=%d" % (W, n, len(bad)))
    assert not bad, "program, error qubits, Pauli index, expected state, states seen: %s" % (bad[:6],)


# ---- through the host path: what the backend hands the engine for a circuit under a noise model ----------------------------------

@pytest.mark.parametrize("j", [0, 1, 2, 5])
def test_lowered_reference_graph_every_word(j):
    case = nc.lowered_case(j)
    assert (case["rec"]["kind"] == _lib.OP_PAULI).sum() > 0 and case["readout"] is not None
    run_case(case, "host path", "lowered graph %d (W=%d, %d records)" % (j, case["W"], len(case["rec"])))


def test_constructed_circuit_errors_on_h_and_x_every_word():
    case = nc.constructed_case()
    assert (case["rec"]["kind"] == _lib.OP_PAULI).sum() > 0
    run_case(case, "host path", "constructed graph 2 (W=%d, %d records)" % (case["W"], len(case["rec"])))


# ---- measurement mapping -----------------------------------------------------------------------------------------------------

def test_full_index_and_wide_registers_with_readout():
    case = nc.mapping_case(64)
    meas, ro = case["meas"], case["readout"]
    assert len(meas) == 64 > case["W"] and -1 in meas and len(set(meas)) < len(meas)
    assert (ro == 0.0).any() and (ro == 1.0).any()
    with _lib.Engine(case["W"]) as eng:
        full = run_case(dict(case, meas=None, readout=None), "mapping", "NULL meas_qubits", eng)
        assert full.max() < 2 ** case["W"]
        got = run_case(case, "mapping", "64 bits, -1, repeats, readout with 0.0 and 1.0", eng)
        unmeasured = sum(1 << j for j, q in enumerate(meas) if q < 0)
        assert unmeasured and not (got & np.uint64(unmeasured)).any()         # a certain flip on a bit nothing writes: stays 0
        assert (got >> np.uint64(63)).any()                                   # the top bit is written
        plain = run_case(dict(case, readout=None), "mapping", "64 bits, no readout", eng)
        for j, q in enumerate(meas):                                          # the same basis states under both mappings
            want = (full >> np.uint64(q)) & np.uint64(1) if q >= 0 else np.zeros_like(full)
            assert np.array_equal((plain >> np.uint64(j)) & np.uint64(1), want)
        for n in (1, 6, 33):
            sub = nc.mapping_case(n, seed=n)
            run_case(sub, "mapping", "%d bits" % n, eng)


def test_empty_meas_qubits_gives_all_zero_words():
    """only NULL means "the full index"; a register of no bits records nothing"""
    case = nc.mapping_case(64)
    with _lib.Engine(case["W"]) as eng:
        got = eng.noisy_sample(case["rec"], case["data"], 500, 3, [])
        assert got.shape == (500,) and not got.any()
        got = eng.noisy_sample(case["rec"], case["data"], 500, 3, [], np.zeros((0, 2)))
        assert not got.any()
        assert eng.noisy_sample(case["rec"], case["data"], 500, 3).any()      # NULL: the full index


# ---- seeds and shot ranges ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", nc.SEEDS)
def test_seeds_use_all_64_bits(seed):
    run_case(nc.seed_case(seed), "seeds", "seed %#x" % seed)


def test_high_seed_word_reaches_the_key():
    a, b = nc.seed_case(2 ** 32), nc.seed_case(0)
    with _lib.Engine(a["W"]) as eng:
        wa = eng.noisy_sample(a["rec"], a["data"], a["shots"], a["seed"], a["meas"], a["readout"])
        wb = eng.noisy_sample(b["rec"], b["data"], b["shots"], b["seed"], b["meas"], b["readout"])
    assert not np.array_equal(wa, wb)


def test_grids_shot_counts_and_empty_calls():
    case = nc.seed_case(2 ** 63 + 12345)
    ref = nc.reference_of(case)
    with _lib.Engine(case["W"]) as eng:
        args = (case["rec"], case["data"])
        tail = (case["seed"], case["meas"], case["readout"])
        for grid in (1, 7):                                       # 1500 = 7 x 214 + 2: the last round of the grid is partial
            eng.set_option("noisy_grid", grid)
            check_words(eng.noisy_sample(*args, case["shots"], *tail), *ref, family="shot ranges", label="noisy_grid=%d" % grid)
        odd = eng.noisy_sample(*args, 1237, *tail)
        check_words(odd, *(r[:1237] for r in ref), family="shot ranges", label="1237 shots, noisy_grid=7")
        eng.set_option("noisy_grid", 0)
        none = eng.noisy_sample(*args, 0, *tail)
        assert none.shape == (0,) and none.dtype == np.uint64
        # an empty program: every word is the mapping of index 0 (with its readout flips)
        rec0, data0 = program.encode([])
        ref0 = exact_noisy_sample(rec0, data0, case["W"], 1000, *tail)
        check_words(eng.noisy_sample(rec0, data0, 1000, *tail), *ref0, family="shot ranges", label="empty program, readout")
        assert not eng.noisy_sample(rec0, data0, 1000, case["seed"], case["meas"]).any()
        assert not eng.noisy_sample(rec0, data0, 1000, case["seed"]).any()
    # more shots than the chip holds workgroups at once: several rounds of the default grid, the last one partial
    W = 2
    rec, data = program.encode(nc.random_ops(W, 222, n_random=12))
    big = dict(W=W, rec=rec, data=data, shots=100003, seed=2 ** 33 + 1, meas=[1, 0, -1], readout=np.array([[0.1, 0.2], [0.0, 1.0], [1.0, 1.0]]))
    run_case(big, "shot ranges", "100003 shots, default grid")


# ---- the draw counter advances on identity draws too ------------------------------------------------------------------------------

def test_identity_heavy_stream():
    case = nc.identity_heavy_case()
    run_case(case, "identity-heavy", "24 x (P(I) = 0.999, P(I) = 0)")

