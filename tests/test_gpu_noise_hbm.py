"""Noisy shots with the trajectories in device memory (qsv_noisy_sample_hbm, qsv_noise_hbm.hip) on the MI355X, word by word.

Up to 13 qubits the slot path runs the cases of the LDS path against the same cached references and against the LDS path
itself; above, random programs with Kraus records at W = 14, 16, 17 against the wide reference (_wide_reference.py), and
forced Paulis (W = 20), forced channels (W = 18) and the cap (W = 24) against plain basis states.  Every word comparison
goes through ``check_words`` / ``check_kraus_words``; test_wide_reference.py asserts on the host that the wide cases have no
ambiguous shot at all."""
import functools

import numpy as np
import pytest

import _kraus_cases as kc
import _noise_exact_cases as nc
import _wide_reference as wr
from _kraus_reference import check_kraus_words
from _noise_exact_cases import check_words
from qcmrf_amd import _lib, ir, program

pytestmark = pytest.mark.gpu

GRIDS = (1, 7)


def sample(eng, c, shots=None):
    return eng.noisy_sample_hbm(c["rec"], c["data"], c["shots"] if shots is None else shots, c["seed"], c["meas"], c["readout"])


@functools.lru_cache(maxsize=None)
def pauli_reference(key):
    """(case, reference) of a Pauli-only case of _noise_exact_cases: computed once, shared, left unchanged"""
    kind, arg = key
    case = {"width": nc.width_case, "seed": nc.seed_case, "mapping": nc.mapping_case}[kind](arg)
    ref = nc.reference_of(case)
    for a in ref:
        a.setflags(write=False)
    return case, ref


def over_grids(eng, c, check, grids=GRIDS):
    for grid in grids + (0,):
        eng.set_option("noisy_grid", grid)
        check(sample(eng, c), "noisy_grid=%d" % grid)
    eng.set_option("noisy_grid", 0)


# ---- the cases of the LDS path through the slot path ---------------------------------------------------------------------

@pytest.mark.parametrize("W", nc.WIDTHS)
def test_pauli_width_cases_every_word(W):
    case, ref = pauli_reference(("width", W))
    with _lib.Engine(W) as eng:
        over_grids(eng, case, lambda got, label: check_words(got, *ref, family="hbm widths", label="W=%d %s" % (W, label)))


@pytest.mark.parametrize("seed", nc.SEEDS)
def test_pauli_seeds_up_to_2_64(seed):
    case, ref = pauli_reference(("seed", seed))
    with _lib.Engine(case["W"]) as eng:
        over_grids(eng, case, lambda got, label: check_words(got, *ref, family="hbm seeds", label="%#x %s" % (seed, label)))


def test_64_bit_register_with_unwritten_bits_and_readout_0_and_1():
    case, ref = pauli_reference(("mapping", 64))
    meas, ro = case["meas"], case["readout"]
    assert len(meas) == 64 and -1 in meas and (ro == 0.0).any() and (ro == 1.0).any()
    with _lib.Engine(case["W"]) as eng:
        over_grids(eng, case, lambda got, label: check_words(got, *ref, family="hbm mapping", label=label))
        got = sample(eng, case)
        unmeasured = sum(1 << j for j, q in enumerate(meas) if q < 0)
        assert unmeasured and not (got & np.uint64(unmeasured)).any()
        assert (got >> np.uint64(63)).any()
        assert not eng.noisy_sample_hbm(case["rec"], case["data"], 200, 3, []).any()        # no bits: all-zero words
        assert eng.noisy_sample_hbm(case["rec"], case["data"], 0, 3).size == 0


@pytest.mark.parametrize("name", list(kc.GPU_CASES))
def test_kraus_cases_every_word(name):
    c, ref = kc.case(name), kc.reference(name)
    with _lib.Engine(c["W"]) as eng:
        over_grids(eng, c, lambda got, label: check_kraus_words(got, *ref, family="hbm kraus", label="%s %s" % (name, label)))


@pytest.mark.parametrize("W", [6, 10, 13])
def test_lds_path_and_slot_path_agree_shot_by_shot(W):
    name = "W=%d" % W
    c = kc.case(name)
    _, _, amb, undet = kc.reference(name)
    with _lib.Engine(W) as eng:
        lds = eng.noisy_sample(c["rec"], c["data"], c["shots"], c["seed"], c["meas"], c["readout"])
        hbm = sample(eng, c)
        again = sample(eng, c)
    assert np.array_equal(hbm, again)
    sure = ~(amb | undet)
    assert sure.sum() >= c["shots"] - nc.ambiguity_cap(c["shots"])
    bad = np.flatnonzero((lds != hbm) & sure)
    assert bad.size == 0, "W=%d: %d shots differ between the paths, first %d: lds %#x, hbm %#x" % (
        W, bad.size, bad[0], int(lds[bad[0]]), int(hbm[bad[0]]))


def test_other_kinds_are_unsupported_and_bad_records_refused():
    with _lib.Engine(3) as eng:
        for op in (ir.op_kq([0, 1], np.eye(4)), ir.op_mux([0], 1, [np.eye(2), np.eye(2)]), ir.Op("swap", a=(0,), b=(1,))):
            r, d = program.encode([op])
            with pytest.raises(RuntimeError, match="-5"):
                eng.noisy_sample_hbm(r, d, 10, 1, [0])
        r, d = program.encode([ir.op_x(3)])
        with pytest.raises(ValueError):
            eng.noisy_sample_hbm(r, d, 10, 1)
        r, d = program.encode([ir.op_x(0)])
        with pytest.raises(ValueError):
            eng.noisy_sample_hbm(r, d, 10, 1, [3])


# ---- wide cases: the first size LDS cannot hold, the last whose qubits fit 4 bits, the first qubit 16 ------------------------

@pytest.mark.parametrize("name", list(wr.WIDE_CASES))
def test_wide_cases_every_word(name):
    c, ref = wr.case(name), wr.reference(name)
    kinds = set(int(k) for k in c["rec"]["kind"])
    assert {_lib.OP_1Q, _lib.OP_MCX, _lib.OP_DIAG, _lib.OP_MCPHASE, _lib.OP_PAULI, _lib.OP_KRAUS} <= kinds
    with _lib.Engine(c["W"]) as eng:
        over_grids(eng, c, lambda got, label: check_kraus_words(got, *ref, family="hbm wide", label="%s %s" % (name, label)),
                   grids=(1, 3))                                  # 48, 12 and 8 shots over 3 workgroups: the last round is partial
        half = c["shots"] // 2
        check_kraus_words(sample(eng, c, half), *(r[:half] for r in ref), family="hbm wide", label="%s first %d shots" % (name, half))
        if c["meas"] is None:
            assert sample(eng, c).max() < 2 ** c["W"]


# ---- a diagonal over more than 8 qubits: list positions 8..15 sit in the record's second word ----------------------------------

def long_diag_program(W, k, b):
    """H on every qubit, DIAG over a seeded permutation of k qubits with table[j] = (-1)^(bit b of j), H on every qubit:
    the state ends in 1 << qubits[b], whatever is drawn"""
    qubits = [int(q) for q in np.random.default_rng(5).permutation(W)[:k]]
    table = 1.0 - 2.0 * ((np.arange(2 ** k) >> b) & 1)
    hs = [ir.op_u(q, kc._H) for q in range(W)]
    return program.encode(hs + [ir.op_diag(qubits, table.astype(complex))] + hs), 1 << qubits[b]


@pytest.mark.parametrize("W,k,b", [(13, 13, 0), (13, 13, 7), (13, 13, 8), (13, 13, 12), (16, 16, 8), (16, 16, 15)])
def test_diag_over_more_than_8_qubits_reads_the_second_word(W, k, b):
    (rec, data), want = long_diag_program(W, k, b)
    assert int(rec["n"][W]) == k > 8
    with _lib.Engine(W) as eng:
        paths = [("hbm", eng.noisy_sample_hbm)] + ([("lds", eng.noisy_sample)] if W <= 13 else [])
        for name, fn in paths:
            for grid in (1, 0):
                eng.set_option("noisy_grid", grid)
                got = fn(rec, data, 8, 23)
                assert (got == want).all(), "%s noisy_grid=%d: expected %#x, states seen %s" % (
                    name, grid, want, sorted(set(int(g) for g in got))[:4])


# ---- forced Paulis at W = 20: plain equality ------------------------------------------------------------------------------------

@pytest.mark.parametrize("qubits", [(0,), (16,), (19,), (19, 0), (0, 19), (16, 15), (15, 16)])
def test_forced_paulis_at_20_qubits_end_in_their_mask(qubits):
    W, shots, bad = 20, 8, []
    with _lib.Engine(W) as eng:
        for p in range(1, 4 ** len(qubits)):
            for which, ((rec, data), want) in zip(("P|0>", "H P H|0>"), nc.forced_pauli_programs(W, qubits, p)):
                got = eng.noisy_sample_hbm(rec, data, shots, 17 + p)
                if not (got == want).all():
                    bad.append((which, p, want, sorted(set(int(g) for g in got))[:4]))
    assert not bad, "qubits %s: program, Pauli index, expected state, states seen: %s" % (qubits, bad[:6])


# ---- forced channels at W = 18 ---------------------------------------------------------------------------------------------------

def forced_channel_programs(W, qs):
    """as kc.forced_programs, on the qubits ``qs``"""
    damp = kc._stack(kc.amplitude_damping_error(1.0))
    r0, r1 = kc._stack(kc.reset_error(1.0)), kc._stack(kc.reset_error(0.0, 1.0))
    ones = sum(1 << q for q in qs)
    hs = [ir.op_u(q, kc._H) for q in range(W)]
    yield "X then damping 1", program.encode([ir.op_x(q) for q in qs] + [kc.kraus_op(q, damp) for q in qs]), 0
    yield "H then reset to 0", program.encode(hs + [kc.kraus_op(q, r0) for q in range(W)]), 0
    yield "reset to 1", program.encode([kc.kraus_op(q, r1) for q in qs]), ones
    yield "H then reset to 1", program.encode(hs + [kc.kraus_op(q, r1) for q in qs]
                                              + [kc.kraus_op(q, r0) for q in range(W) if q not in qs]), ones


def test_forced_channels_at_18_qubits_end_in_their_state():
    W, bad = 18, []
    with _lib.Engine(W) as eng:
        for label, (rec, data), want in forced_channel_programs(W, (0, 16, 17)):
            got = eng.noisy_sample_hbm(rec, data, 8, 23)
            if not (got == want).all():
                bad.append((label, want, sorted(set(int(g) for g in got))[:4]))
    assert not bad, "program, expected state, states seen: %s" % (bad,)


# ---- the cap ------------------------------------------------------------------------------------------------------------------------

def test_24_qubits_run_and_25_are_refused():
    rec, data = program.encode([ir.op_x(23), ir.op_x(0)])
    with _lib.Engine(24) as eng:
        got = eng.noisy_sample_hbm(rec, data, 2, 5)
    assert got.tolist() == [2 ** 23 + 1] * 2
    with _lib.Engine(25) as eng:
        with pytest.raises(ValueError, match="24"):
            eng.noisy_sample_hbm(rec, data, 2, 5)
