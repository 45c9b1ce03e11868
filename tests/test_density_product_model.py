"""The references of tests/test_gpu_density_forms.py on the host: the product of pair factors of ``pair_program_k2`` is the
rho of the interleaved program; the comparisons the GPU tests make can fail -- each of four wrong references differs from the
true one by more than 1e-6 where the GPU tests look (1e-6 separates such errors from rounding; it is no tolerance of the
engine) --; the reference of the big sampling case stays within the ambiguity cap on its own."""
import numpy as np
import pytest

import _density_cases as dc
import _kraus2_cases as k2c
import _noise_exact_cases as nc
from _kraus2_reference import kraus2_rho
from qcmrf_amd import _lib
from test_gpu_density import AMP_TOL

SEPARATION = 1e-6
WIDE = [(11, False), (13, False), (14, False), (16, True)]          # (W, short) of the GPU tests' product programs


@pytest.mark.parametrize("W", [6, 7])
def test_product_of_factors_is_the_rho_of_the_interleaved_program(W):
    c = dc.k2_case(W)
    N = 1 << W
    rho = kraus2_rho(c["rec"], c["data"], W)
    i, j = np.arange(N)[:, None], np.arange(N)[None, :]
    err = float(np.abs(dc.product_entries(c["factors"], W, i, j) - rho).max())
    print("DENSITY product model W=%d: %d records, max |product - rho| = %.3g" % (W, len(c["rec"]), err))
    assert err <= AMP_TOL
    assert float(np.abs(dc.product_vector(c["factors"], W) - dc.vec_of(rho)).max()) <= AMP_TOL
    assert np.abs(dc.product_diagonal(c["factors"], W) - np.real(np.diag(rho))).max() <= AMP_TOL
    cols = dc.column_set(W)
    assert np.abs(dc.product_columns(c["factors"], W, cols) - rho[:, cols].T).max() <= AMP_TOL


@pytest.mark.parametrize("W,short", WIDE + [(6, False)])
def test_programs_hold_what_the_gpu_tests_need(W, short):
    c = dc.k2_case(W, short)
    pairs = [tuple(q % W for q in p) for p in dc.K2_PAIRS[W]]
    k2 = [o for o in c["ops"] if o.kind == "kraus2"]
    placed = {tuple(o.qubits) for o in k2}
    assert (0, W - 1) in placed and any(abs(a - b) == 1 for a, b in placed)
    if W <= 11:
        assert any(q + W == 11 for p in placed for q in p)          # a bra bit on address bit 11
    for o in c["ops"]:                                              # entanglement and two-qubit channels stay inside a pair
        qs = set(o.qubits) if o.kind in dc.CHANNELS else {o.target, *o.ctrls} if o.kind in ("u", "x") else set()
        assert len(qs) <= 1 or any(qs == set(p) for p in pairs), str(o)
    kinds = [o.kind for o in c["ops"]]
    if short:
        assert len(c["ops"]) <= 16
        for pair in ((0, W - 1), pairs[1]):
            for kind in ("kraus2", "pauli"):
                assert sum(o.kind == kind and set(o.qubits) == set(pair) for o in c["ops"]) == 1
        for q in (0, W - 1):
            for kind in ("kraus", "pauli"):
                assert sum(o.kind == kind and tuple(o.qubits) == (q,) for o in c["ops"]) == 1
    else:
        assert {(b, a) for a, b in placed} == placed                # every pair in both orders
        assert {len(o.table) for o in k2} >= {1, 2, 4, 16}
        if len(pairs) >= 3:
            assert len(k2) >= len(k2c.menu(np.random.RandomState(0)))    # the whole menu
        assert all(kind in kinds for kind in ("u", "x", "pauli", "kraus", "kraus2"))
    assert any(j >> (W - 1) for j in dc.column_set(W)) and len(set(dc.column_set(W))) >= W + 2


@pytest.mark.parametrize("wrong", dc.K2_WRONG)
@pytest.mark.parametrize("W,short", WIDE)
def test_wrong_references_differ_on_the_column_set(W, short, wrong):
    cols = dc.column_set(W)
    true = dc.product_columns(dc.k2_case(W, short)["factors"], W, cols)
    diff = float(np.abs(dc.product_columns(dc.k2_wrong_factors(W, wrong, short), W, cols) - true).max())
    print("DENSITY product model W=%d: %s differs by %.3g on the column set (largest entry %.3g)" % (W, wrong, diff, np.abs(true).max()))
    assert diff > SEPARATION


@pytest.mark.parametrize("wrong", dc.K2_WRONG)
def test_wrong_references_differ_on_the_whole_vector_of_w11(wrong):
    diff = float(np.abs(dc.product_vector(dc.k2_wrong_factors(11, wrong), 11) - dc.k2_vector(11)).max())
    print("DENSITY product model W=11: %s differs by %.3g on the vector" % (wrong, diff))
    assert diff > SEPARATION


@pytest.mark.parametrize("W", [2, 3, 7])
def test_wrong_references_differ_on_the_small_whole_vector_cases(W):
    """the forced-form cases ``_kraus2_cases.case("W=%d")``: the KRAUS2 records with their qubits swapped, conjugated operators
    and the transposed rho (these programs are no products: no factor to leave out)"""
    c = k2c.case("W=%d" % W)
    rec, data = c["rec"], c["data"]
    rho = kraus2_rho(rec, data, W)
    k2 = np.flatnonzero(rec["kind"] == _lib.OP_KRAUS2)
    swapped = rec.copy()
    swapped["qubits"][k2, :2] = rec["qubits"][k2, 1::-1]           # as a kernel that takes the two qubits the wrong way round does
    conj = np.array(data, dtype=np.float64, copy=True)
    for r in rec[(rec["kind"] == _lib.OP_KRAUS2) | (rec["kind"] == _lib.OP_KRAUS)]:
        n = (32 if r["kind"] == _lib.OP_KRAUS2 else 8) * int(r["vals"][0])
        conj[int(r["data_off"]) + 1:int(r["data_off"]) + n:2] *= -1.0
    for label, other in (("swapped", kraus2_rho(swapped, data, W)), ("conjugated", kraus2_rho(rec, conj, W)), ("transposed", rho.T)):
        diff = float(np.abs(other - rho).max())
        print("DENSITY product model %s of case W=%d differs by %.3g" % (label, W, diff))
        assert diff > SEPARATION, label


def test_big_sampling_reference_stays_within_the_ambiguity_cap():
    c, words, alt, amb, diag = dc.big_sample_reference()
    assert c["shots"] > 4096 * 256 and c["seed"] >= 2 ** 32 and -1 in c["meas"] and c["readout"] is not None
    assert abs(diag.sum() - 1.0) <= AMP_TOL and (diag > 0.05).all()
    print("DENSITY big sample: %d shots, %d ambiguous (cap %d)" % (words.size, int(amb.sum()), nc.ambiguity_cap(words.size)))
    assert int(amb.sum()) <= nc.ambiguity_cap(words.size)
    assert set(int(w) for w in np.unique(words)) == {0, 1, 4, 5} and np.array_equal(words[~amb], alt[~amb])
