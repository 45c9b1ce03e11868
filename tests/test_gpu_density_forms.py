"""The density-matrix kernels on the MI355X in the forms that only wide registers or engine options select, against the numpy
rho (``numpy_rho`` / ``kraus2_rho``) and, past the widths numpy can hold, against the Kronecker product of pair factors of
``_density_cases.pair_program_k2`` (test_density_product_model.py shows on the host that the product is the rho of the
program and that the comparisons made here see a swapped KRAUS2 record, conjugated operators, a transposed rho and a
factor without its channels).

Which test catches what (each reverted in a scratch build is a named failure here):
  the NT template argument of k_dm_kraus2 / k_dm_kraus / k_dm_pauli used wrongly (the non-temporal instantiations ran in no
      test for KRAUS2, in one test on five columns for the others)       a: test_forced_nontemporal_whole_vector,
                                                                          b: test_grid_stride_whole_vector_w11[1],
                                                                          c: test_forms_chosen_by_size[W=13 by size], [W=14 by size]
  ``t += gridDim.x * QSV_TPB`` of a channel kernel replaced by a break    b: test_grid_stride_whole_vector_w11 (and the
                                                                          W = 13 case of c with blocks_per_cu = 1)
  a 32-bit ``off[]`` in a channel kernel (``int``: bit 31 is its sign), a 32-bit block number in ``dm_base`` or
      ``1 << pos`` in ``dm_offset``, a 32-bit i in ``k_dm_diag``           d: test_w16_vector_of_2_to_the_32_entries
      (an ``unsigned`` ``off[]`` still holds every offset of W = 16: 2^32 - 1 at most; only W = 17, 256 GiB, would see it)
  ``k_dm_sample`` dropping the shots past its grid of 4096 workgroups     e: test_sample_past_the_grid_cap
  ``density_sample`` (or a KRAUS2 record, or ``noisy_sample``) reusing a stale ``d_noisy`` capacity or pointer, ``d_red``
      after another entry point reallocated it                            f: test_entry_points_interleaved_on_one_handle

Tolerances are the project's two promises, those of test_gpu_density.py: AMP_TOL on amplitudes, PROB_TOL on probabilities;
word comparisons go through ``check_words`` with its cap."""
import functools

import numpy as np
import pytest

import _density_cases as dc
import _kraus2_cases as k2c
import _noise_exact_cases as nc
from _kraus2_reference import kraus2_rho
from qcmrf_amd import _lib, program
from test_gpu_density import AMP_TOL, PROB_TOL, check_state

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def small_case(name):
    """(W, rec, data, rho) of a forced-form case; rho computed once, shared, left unchanged"""
    kind, W = name.split()
    W = int(W)
    if kind == "kraus2":
        c = k2c.case("W=%d" % W)
        rho = kraus2_rho(c["rec"], c["data"], W)
        rho.setflags(write=False)
        return W, c["rec"], c["data"], rho
    return (W,) + dc.width_case(W)


def channel_records(rec):
    return int(np.isin(rec["kind"], (_lib.OP_PAULI, _lib.OP_KRAUS, _lib.OP_KRAUS2)).sum())


def check_booking(eng, rec, W):
    """every PAULI, KRAUS and KRAUS2 record was one launch booked as QSV_K_KQ with 32 B per amplitude (dm_channel)"""
    kq = eng.stats()["kinds"]["kq"]
    assert kq["launches"] == channel_records(rec)
    assert kq["bytes"] == 32.0 * 4.0 ** W * channel_records(rec)


def check_diagonals(eng, factors, W, sizes):
    """trace, the full diagonal and partial diagonals over ``sizes`` permuted qubits; returns the worst error"""
    diag = dc.product_diagonal(factors, W)
    rng = np.random.RandomState(300 + W)
    full, trace = eng.density_diagonal(list(range(W)))
    worst = float(np.abs(full - diag).max())
    assert abs(trace - 1.0) <= AMP_TOL, trace
    for k in sizes:
        qs = [int(q) for q in rng.permutation(W)[:k]]
        m, tr = eng.density_diagonal(qs)
        assert tr == trace
        worst = max(worst, float(np.abs(m - dc.marginal(diag, qs)).max()))
    assert worst <= PROB_TOL
    return worst, abs(trace - 1.0)


def check_columns(eng, factors, W):
    """rho[:, j] for the column set: j = 0, 2^W - 1, every single bit, 16 random; returns the worst error"""
    cols = dc.column_set(W)
    want = dc.product_columns(factors, W, cols)
    worst = 0.0
    for c, j in enumerate(cols):
        got = eng.amplitudes(j << W, 1 << W)
        err = float(np.abs(got - want[c]).max())
        assert err <= AMP_TOL, (j, err)
        worst = max(worst, err)
    return worst


# ---- a. non-temporal forms forced at small widths ----------------------------------------------------------------------------------

@pytest.mark.parametrize("nt", [0, 1])
@pytest.mark.parametrize("name", ["kraus2 2", "kraus2 3", "kraus2 7", "width 5", "width 6"])
def test_forced_nontemporal_whole_vector(name, nt):
    """every channel kernel in both instantiations (``nontemporal`` = 0, 1) at the smallest shapes where a wrong offset
    table of one of them shows: whole vector, Hermiticity, trace, full and permuted partial diagonals"""
    W, rec, data, rho = small_case(name)
    with _lib.Engine(2 * W) as eng:
        eng.set_option("nontemporal", nt)
        eng.density_exec(rec, data)
        check_state(eng, rho, W, "forms nontemporal=%d %s" % (nt, name))
        check_booking(eng, rec, W)


# ---- b. later iterations of the grid-stride loops ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("nt", [0, 1])
def test_grid_stride_whole_vector_w11(nt):
    """blocks_per_cu = 1: a grid of n_cu workgroups.  A KRAUS2 record has 4^11 / 16 = 262144 blocks: 4 per thread on 256
    CUs (2 on a device of 512), a one-qubit record 16.  W = 11 is the smallest width at which k_dm_kraus2 strides at all.
    All 4^11 entries against the product of factors, the full and three partial diagonals, the launches booked"""
    W = 11
    c = dc.k2_case(W)
    with _lib.Engine(2 * W) as eng:
        eng.set_option("blocks_per_cu", 1)
        eng.set_option("nontemporal", nt)
        eng.density_exec(c["rec"], c["data"])
        check_booking(eng, c["rec"], W)
        got = eng.amplitudes()
        err = float(np.abs(got - dc.k2_vector(W)).max())
        G = got.reshape(1 << W, 1 << W)
        herm = float(np.abs(G - G.conj().T).max())
        perr, terr = check_diagonals(eng, c["factors"], W, (6, 10, 3))
    print("DENSITY forms grid stride nontemporal=%d: W=%d max |amp - reference| = %.3g over 4^%d entries, Hermiticity %.3g, "
          "max |p - reference| = %.3g, |trace - 1| = %.3g" % (nt, W, err, W, herm, perr, terr))
    assert err <= AMP_TOL and herm <= AMP_TOL


# ---- c. the forms chosen by size -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W,options", [(13, ()), (13, (("nontemporal", 0), ("blocks_per_cu", 1))), (14, ())],
                         ids=["W=13 by size", "W=13 temporal capped", "W=14 by size"])
def test_forms_chosen_by_size(W, options):
    """W = 13 and 14 with default options are non-temporal by size (2W >= 26); W = 13 with nontemporal = 0 and one workgroup
    per CU walks 64 KRAUS2 blocks per thread.  Trace, diagonals, and the column set: every bra bit both ways, and the
    blocks that only late loop iterations reach"""
    c = dc.k2_case(W)
    with _lib.Engine(2 * W) as eng:
        for name, value in options:
            eng.set_option(name, value)
        eng.density_exec(c["rec"], c["data"])
        check_booking(eng, c["rec"], W)
        perr, terr = check_diagonals(eng, c["factors"], W, (6, 10))
        err = check_columns(eng, c["factors"], W)
    print("DENSITY forms by size %s: W=%d max |amp - reference| = %.3g over %d columns, max |p - reference| = %.3g, |trace - 1| = %.3g"
          % (dict(options), W, err, len(dc.column_set(W)), perr, terr))


# ---- d. W = 16 ------------------------------------------------------------------------------------------------------------------------

def test_w16_vector_of_2_to_the_32_entries():
    """a 64 GiB state: the bra bit of qubit 15 is address bit 31, so an ``int`` or ``unsigned`` in a block count, shift or
    offset gives wrong amplitudes here and nowhere below.  A short program (each record is a sweep of 128 GB): KRAUS2 and
    two-qubit PAULI on (0, 15) and on (5, 6), one-qubit KRAUS and PAULI on qubits 15 and 0.  The column set holds
    j = 2^15 and j = 2^16 - 1: address bit 31 set"""
    W = 16
    free, _ = _lib.device_memory(0)
    if free < 70 * 2 ** 30:
        pytest.skip("needs 70 GiB of free device memory, %.0f GiB are free" % (free / 2 ** 30))
    c = dc.k2_case(W, True)
    assert len(c["rec"]) <= 16 and any(j >> 15 for j in dc.column_set(W))
    with _lib.Engine(2 * W) as eng:
        eng.density_exec(c["rec"], c["data"])
        check_booking(eng, c["rec"], W)
        perr, terr = check_diagonals(eng, c["factors"], W, (6, 10))
        err = check_columns(eng, c["factors"], W)
    print("DENSITY forms W=16: max |amp - reference| = %.3g over %d columns, max |p - reference| = %.3g, |trace - 1| = %.3g"
          % (err, len(dc.column_set(W)), perr, terr))


# ---- e. k_dm_sample past its grid cap -----------------------------------------------------------------------------------------------

def test_sample_past_the_grid_cap():
    """2^20 + 777 shots: more than the 4096 x 256 threads of k_dm_sample's grid, so its loop runs a second time; seed above
    2^32, permuted register with an unused bit, readout errors; every word.  A shot depends on (seed, shot) alone: a call of
    1000 shots gives the first 1000 words"""
    c, words, alt, amb, diag = dc.big_sample_reference()
    with _lib.Engine(2 * c["W"]) as eng:
        eng.density_exec(c["rec"], c["data"])
        got = eng.density_sample(c["shots"], c["seed"], c["meas"], c["readout"])
        first = eng.density_sample(1000, c["seed"], c["meas"], c["readout"])
        full, _ = eng.density_diagonal(list(range(c["W"])))
    assert np.abs(full - diag).max() <= PROB_TOL
    nc.check_words(got, words, alt, amb, family="density sample", label="2^20 + 777 shots")
    assert np.array_equal(got[:1000], first)


# ---- f. entry points interleaved on one handle -----------------------------------------------------------------------------------------

def test_entry_points_interleaved_on_one_handle():
    """``d_noisy`` holds a KRAUS2 superoperator, then ``density_sample``'s tables and words, then ``noisy_sample``'s program;
    ``d_red`` the diagonal and the cumulative sums, then the scratch of ``probabilities`` and ``expect_diag``, which
    reallocate it.  Every result on the one handle must equal, bit for bit, what a fresh handle returns for that call"""
    W = 6
    A, B = dc.k2_case(W), dc.k2_case(W, False, 4242)
    noisy = program.encode(k2c.random_ops(2 * W, 7012, 12))
    rho = kraus2_rho(A["rec"], A["data"], W)
    meas, ro = [3, 0, -1, 5, 1, 2, 4], np.tile([0.03, 0.06], (W + 1, 1))
    table = np.random.RandomState(12).randn(1 << (2 * W))
    all12 = list(range(2 * W))

    def fresh(prog, call):
        with _lib.Engine(2 * W) as e:
            if prog is not None:
                e.density_exec(prog["rec"], prog["data"])
            return call(e)

    def same(a, b):
        a, b = (a if isinstance(a, tuple) else (a,)), (b if isinstance(b, tuple) else (b,))
        return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))

    calls = {"diagonal": lambda e: e.density_diagonal(list(range(W))),
             "sample 6000": lambda e: e.density_sample(6000, 2 ** 33 + 9, meas, ro),
             "probabilities": lambda e: e.probabilities(all12),
             "expect_diag": lambda e: e.expect_diag(all12, table),
             "amplitudes": lambda e: e.amplitudes(),
             "sample 200000": lambda e: e.density_sample(200000, 2 ** 33 + 9, meas, ro),
             "noisy_sample": lambda e: e.noisy_sample(noisy[0], noisy[1], 300, 77)}
    steps = [(A, "amplitudes"), (None, "diagonal"), (None, "sample 6000"), (None, "probabilities"), (None, "expect_diag"),
             (B, "amplitudes"), (None, "sample 200000"), (None, "noisy_sample"), (A, "amplitudes"), (None, "diagonal"),
             (None, "sample 6000")]
    with _lib.Engine(2 * W) as eng:
        state, results = None, []
        for n, (prog, name) in enumerate(steps):
            if prog is not None:
                eng.density_exec(prog["rec"], prog["data"])
                state = prog
            got = calls[name](eng)
            results.append(got)
            want = fresh(None if name == "noisy_sample" else state, calls[name])
            assert same(got, want), "step %d (%s) differs from a fresh handle" % (n, name)
    first, last = results[0], results[8]
    err = float(np.abs(last - dc.vec_of(rho)).max())
    print("DENSITY forms interleaved: W=%d %d calls on one handle equal a fresh handle's bit for bit, max |amp - reference| = %.3g"
          % (W, len(steps), err))
    assert np.array_equal(first, last) and err <= AMP_TOL
    assert same(results[1], results[9]) and same(results[2], results[10])
    assert np.abs(results[1][0] - np.real(np.diag(rho))).max() <= PROB_TOL
