"""CPU: post-selected sampling.  The exact reference of ``qsv_sample_cond`` pinned (and two wrong samplers rejected), the
compact index map and the deferred tile list restated in numpy and checked by enumeration, and the backend's
``post_select`` logic on the numpy stand-in engine (``_post_select_cases.CondNumpyEngine``)."""
import itertools
import json
import math
import os

import numpy as np
import pytest

import _post_select_cases as pc
import _sampler_cases as sc
from _sampler_reference import TOL_REL, check_inverse_cdf, exact_index_order, rules_of, sorted_uniforms
from conftest import random_theta
from qcmrf_amd import QCMRF, mrf, workloads
from qcmrf_amd.backend import QsvBackend
from qcmrf_amd.qcmrf import extract_probs


def _state(n, seed):
    return sc.probs(sc.rand_state(n, seed))


# ---- the reference --------------------------------------------------------------------------------------------------
def test_mask_zero_is_the_unconditioned_reference():
    p = _state(8, 3)
    want, dist, r, mass = pc.conditional_reference(p, 0, 0, 17, 500)
    total = math.fsum(p.tolist())
    r0 = sorted_uniforms(17, 500, total)
    w0, d0 = exact_index_order(p, r0)
    assert mass == total and np.array_equal(r, r0) and np.array_equal(want, w0) and np.array_equal(dist, d0)


@pytest.mark.parametrize("fix", [(0b100000, 0b100000), (0b001001, 0b000001), (0b111000, 0b010000)])
def test_every_word_matches_and_the_histogram_follows_the_masked_p(fix):
    fm, fv = fix
    p = _state(6, 5)
    shots = 200000
    want, dist, r, mass = pc.conditional_reference(p, fm, fv, 23, shots)
    assert ((want & np.uint64(fm)) == np.uint64(fv)).all()
    pm = np.where(pc.match_of(p.size, fm, fv), p, 0.0)
    assert abs(mass - math.fsum(pm.tolist())) == 0
    assert check_inverse_cdf(pm, r, want, TOL_REL * mass, mass) == []
    obs = np.bincount(want.astype(np.int64), minlength=p.size)
    sel = pm > 0
    assert obs[~sel].sum() == 0 and (obs[sel] > 0).all()
    # every count within six binomial standard deviations of its expectation
    q = pm[sel] / mass
    assert (np.abs(obs[sel] - q * shots) < 6 * np.sqrt(shots * q * (1 - q)) + 1).all()


def test_two_wrong_samplers_are_rejected():
    """shots normalised by the total instead of the conditional mass; the mask applied after an unconditioned draw"""
    p = _state(6, 5)
    fm, fv = 0b100100, 0b000100
    shots = 4000
    want, dist, r, mass = pc.conditional_reference(p, fm, fv, 9, shots)
    pm = np.where(pc.match_of(p.size, fm, fv), p, 0.0)
    tol = TOL_REL * mass
    assert check_inverse_cdf(pm, r, want, tol, mass) == []
    # (a) uniforms scaled to the whole norm, walked over the masked p: everything past the mass piles on the last index
    total = math.fsum(p.tolist())
    ra = sorted_uniforms(9, shots, total)
    xa, _ = exact_index_order(pm, ra)
    assert not np.array_equal(xa, want)
    assert rules_of(check_inverse_cdf(pm, r, xa, tol, mass)) != []
    # (b) an unconditioned draw, shots that miss the mask dropped: fewer words, and not the words of the contract
    xb_all, _ = exact_index_order(p, ra)
    xb = xb_all[(xb_all & np.uint64(fm)) == np.uint64(fv)]
    assert len(xb) < shots
    assert rules_of(check_inverse_cdf(pm, r[:len(xb)], xb, tol, mass)) != []


# ---- the compact index space ------------------------------------------------------------------------------------------
def test_compact_map_enumerates_the_matching_indices_in_ascending_order():
    bits = 10
    g = np.arange(1 << bits, dtype=np.uint64)
    n = 0
    for k in range(4):
        for F in itertools.combinations(range(bits), k):
            fm = sum(1 << q for q in F)
            for vals in itertools.product((0, 1), repeat=k):
                fv = sum(v << q for q, v in zip(F, vals))
                got = pc.compact_addresses(bits, F, fv)
                assert np.array_equal(got, g[(g & np.uint64(fm)) == np.uint64(fv)]), (F, vals)
                n += 1
    assert n == 1 + 10 * 2 + 45 * 4 + 120 * 8


# ---- the tile list of a deferred shard ----------------------------------------------------------------------------------
def test_deferred_geometry_is_the_documented_one():
    geo = pc.deferred_geometry()
    assert geo.ntiles == 16 and geo.block_bits() == [7, 8, 9, 10]


def test_tile_list_is_exactly_the_tiles_that_hold_a_matching_address():
    geo = pc.deferred_geometry()
    addr = np.arange(1 << geo.w, dtype=np.uint64)
    tile = geo.tile_of(addr)
    pool = [3, 5, 7, 9, 10, 15]
    for k in range(len(pool) + 1):
        for F in itertools.combinations(pool, k):
            fm = sum(1 << q for q in F)
            for vals in itertools.product((0, 1), repeat=k):
                fv = sum(v << q for q, v in zip(F, vals))
                lst, nfixed = pc.tile_list(geo, fm, fv)
                want = np.unique(tile[(addr & np.uint64(fm)) == np.uint64(fv)])
                assert nfixed == len([q for q in F if q in (7, 8, 9, 10)])
                assert (np.diff(lst.astype(np.int64)) > 0).all()          # ascending, duplicate-free
                assert np.array_equal(lst, want), (F, vals)


# ---- the backend ------------------------------------------------------------------------------------------------------
def _backend(**opts):
    be = QsvBackend(**opts)
    be._engine_factory = pc.factory
    return be


@pytest.mark.parametrize("layout", ["auto", "reference"])
def test_classical_bits_are_translated_to_physical_bits(layout):
    C = [[0, 1], [1, 2], [2, 3]]
    n, m = 4, 3
    qc = QCMRF(C, random_theta(12))
    be = _backend(layout=layout)
    post = qc.post_selection()
    assert post == {5: 0, 6: 0, 7: 0}
    res = be.run(qc, shots=2000, seed_simulator=3, post_select=post).result()
    md = res.metadata(0)
    counts = res.get_counts()
    assert sum(counts.values()) == 2000
    assert all(len(k) == n + m + 1 and k[:m] == "0" * m for k in counts)      # full-width keys, ancilla bits 0
    assert md["post_select"] == post and md["post_select_path"] == "stored"
    # the words are those of the reference on the engine's own amplitudes under the plan's layout
    p = np.abs(be.last_engine.amplitudes()) ** 2
    lay = md["layout"]
    fm = sum(1 << lay[q] for q in post)                                        # classical bit c <- qubit c in a QCMRF circuit
    want, _, _, mass = pc.conditional_reference(p, fm, 0, 3, 2000)
    logical = np.zeros_like(want)
    for q in range(n + m + 1):
        if q != n:
            logical |= ((want >> np.uint64(lay[q])) & np.uint64(1)) << np.uint64(q)
    uv, uc = np.unique(logical, return_counts=True)
    assert counts == {format(int(v), "0%db" % (n + m + 1)): int(c) for v, c in zip(uv, uc)}
    assert abs(md["post_select_probability"] - mass / math.fsum(p.tolist())) < 1e-14
    P, delta = extract_probs(counts, n, m + 1)
    assert delta == 1.0
    # a bit fixed to 1 selects the other branch
    res1 = be.run(qc, shots=500, seed_simulator=3, post_select={5: 1}).result()
    assert all(k[-6] == "1" for k in res1.get_counts())


def test_probability_is_the_success_probability_of_the_seven_reference_graphs():
    be = _backend()
    for j, C in enumerate(workloads.REFERENCE_GRAPHS):
        th = random_theta(mrf.dimension(C))
        qc = QCMRF(C, th)
        md = be.run(qc, shots=0, post_select=qc.post_selection()).result().metadata(0)
        assert abs(md["post_select_probability"] - mrf.success_probability(C, th)) < 1e-12, j


def test_shots_zero_returns_the_probability_and_no_counts():
    C = [[0, 1, 2]]
    qc = QCMRF(C, random_theta(8))
    res = _backend().run(qc, shots=0, post_select=qc.post_selection()).result()
    assert res.get_counts() == {}
    assert 0 < res.metadata(0)["post_select_probability"] < 1


def test_a_list_gives_every_circuit_its_own_dict():
    qa = QCMRF([[0, 1]], random_theta(4))
    qb = QCMRF([[0, 1], [1, 2]], random_theta(8))
    be = _backend()
    res = be.run([qa, qb], shots=300, seed_simulator=1, post_select=[qa.post_selection(), {4: 0, 5: 1}]).result()
    ca, cb = res.get_counts()
    assert all(k[0] == "0" for k in ca)
    assert all(k[0] == "1" and k[1] == "0" for k in cb)
    assert res.metadata(1)["post_select"] == {4: 0, 5: 1}
    with pytest.raises(ValueError):
        be.run([qa, qb], shots=10, post_select=[qa.post_selection()])
    one = be.run([qa, qa], shots=50, seed_simulator=1, post_select=qa.post_selection()).result()
    assert all(k[0] == "0" for c in one.get_counts() for k in c)


def test_refusals():
    from qcmrf_amd import noise
    C = [[0, 1], [1, 2]]
    qc = QCMRF(C, random_theta(8))
    be = _backend()
    with pytest.raises(ValueError, match="no measurement writes"):
        be.run(qc, shots=10, post_select={3: 0})                              # the AND scratch qubit is never measured
    with pytest.raises(ValueError, match="0 or 1"):
        be.run(qc, shots=10, post_select={4: 2})
    with pytest.raises(ValueError, match="method"):
        be.run(qc, shots=10, post_select={4: 0}, method="trajectory")
    with pytest.raises(ValueError, match="method"):
        be.run(qc, shots=10, post_select={4: 0}, method="density_matrix")
    nm = noise.NoiseModel()
    nm.add_all_qubit_readout_error(noise.ReadoutError([[0.9, 0.1], [0.1, 0.9]]))
    with pytest.raises(ValueError, match="noise_model"):
        be.run(qc, shots=10, post_select={4: 0}, noise_model=nm)

    class Two:
        world, rank = 2, 0
    with pytest.raises(ValueError, match="one process"):
        be.run(qc, shots=10, post_select={4: 0}, comm=Two())
    # zero probability: a qubit nothing acts on reads 0 for certain
    from qcmrf_amd.circuit import QuantumCircuit
    qz = QuantumCircuit(2, 2)
    qz.h(0)
    qz.measure(0, 0)
    qz.measure(1, 1)
    with pytest.raises(ValueError, match="zero probability"):
        be.run(qz, shots=10, post_select={1: 1})
    with pytest.raises(ValueError, match="zero probability"):
        be.run(qz, shots=0, post_select={1: 1})


def test_two_classical_bits_of_one_qubit_must_agree():
    from qcmrf_amd.circuit import QuantumCircuit
    qc = QuantumCircuit(2, 3)
    qc.h(0)
    qc.h(1)
    qc.measure(0, 0)
    qc.measure(0, 2)
    qc.measure(1, 1)
    be = _backend()
    with pytest.raises(ValueError, match="both 0 and 1"):
        be.run(qc, shots=10, post_select={0: 0, 2: 1})
    counts = be.run(qc, shots=200, seed_simulator=2, post_select={0: 1, 2: 1}).result().get_counts()
    assert set(counts) <= {"101", "111"} and sum(counts.values()) == 200


def test_post_selection_needs_measurements():
    assert QCMRF([[0, 1], [1, 2]], random_theta(8)).post_selection() == {4: 0, 5: 0}
    with pytest.raises(ValueError):
        QCMRF([[0, 1]], random_theta(4), with_measurements=False).post_selection()


def test_run_experiment_writes_both_files(tmp_path, monkeypatch):
    from qcmrf_amd import Aer, run_experiment
    be = Aer.get_backend("qasm_simulator")
    monkeypatch.setattr(be, "_engine_factory", pc.factory)
    monkeypatch.setattr(be, "_engine", None)
    monkeypatch.setattr(be, "_engine_key", None)
    run_experiment.main(["--post-select", "--reps", "1", "--shots", "200", "--outdir", str(tmp_path), "--seed-simulator", "4"])
    counts = json.load(open(os.path.join(str(tmp_path), "result_simulation_postselected_0.5.json")))
    success = json.load(open(os.path.join(str(tmp_path), "success_simulation_0.5.json")))
    models = json.load(open(os.path.join(str(tmp_path), "models_0.5.json")))
    assert len(counts) == len(success) == len(workloads.REFERENCE_GRAPHS)
    for j, C in enumerate(workloads.REFERENCE_GRAPHS):
        n, m = mrf.num_vertices(C), len(C)
        assert sum(counts[j].values()) == 200
        assert all(len(k) == n + m + 1 and k[:m] == "0" * m for k in counts[j])
        assert isinstance(success[j], float)
        assert abs(success[j] - mrf.success_probability(C, models["THETAS"][str(j)][0])) < 1e-12
