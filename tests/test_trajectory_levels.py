"""CPU: the level-wise walk of the trajectory mode (qcmrf_amd.trajectory, walk="levels") and classical registers past 64
bits, on the numpy engine with the reference slot primitives of _branch_reference.py."""
import json
import os

import numpy as np
import pytest

import _branch_reference as br
from conftest import GOLDEN, random_theta
from oracle import closed_form as cf
from qcmrf_amd import QCMRF, mrf, trajectory, workloads
from qcmrf_amd.backend import QsvBackend

W67_CLIQUES = [[i % 6, (i + 1) % 6] for i in range(60)]      # 6 variables, 60 cliques: W = 67, 8 live qubits
W67_SHOTS = 4000


def w67_circuit():
    return QCMRF(W67_CLIQUES, random_theta(240, 0.05))


def check_w67_counts(counts, shots):
    """keys of 67 characters, bits beyond 63 set, success rate and marginals of the Gibbs distribution"""
    n = 6
    assert sum(counts.values()) == shots and all(len(k) == 67 and set(k) <= {"0", "1"} for k in counts)
    assert any("1" in k[:67 - 64] for k in counts)            # a set bit left of position 64
    assert all(k[67 - 1 - n] == "0" for k in counts)           # the scratch qubit
    pg, lnZ = mrf.gibbs_pmf(W67_CLIQUES, random_theta(240, 0.05))
    delta = float(np.exp(lnZ) / 2 ** n)
    bound = 5 * np.sqrt(delta * (1 - delta) / shots) + 1e-3
    good = {int(k, 2): v for k, v in counts.items() if int(k, 2) < 2 ** n}
    ok = sum(good.values())
    assert abs(ok / shots - delta) < bound, (ok / shots, delta)
    idx = np.arange(2 ** n)
    xs = np.array(sorted(good))
    ws = np.array([good[x] for x in xs.tolist()], dtype=np.float64)
    for j in range(n):
        for sel in (((idx >> j) & 1) == 1, (((idx >> j) & 1) & ((idx >> ((j + 1) % n)) & 1)) == 1):
            hit = ws[sel[xs]].sum()
            # successful shots with the bit(s) set, out of ALL shots: a binomial of probability delta * marginal <= delta
            assert abs(hit / shots - delta * pg[sel].sum()) < bound, j
            # ... and the marginal among the successful shots, as the device test of chain(22) bounds it
            assert abs(hit / ok - pg[sel].sum()) < 5 * 0.5 / np.sqrt(ok) + 1e-3, j


@pytest.mark.parametrize("walk", ["depth", "levels"])
def test_w67_register_past_64_bits(walk):
    be = QsvBackend(method="trajectory")
    be._engine_factory = br.factory
    res = be.run(w67_circuit(), shots=W67_SHOTS, seed_simulator=3, trajectory_walk=walk).result()
    meta = res.metadata(0)
    assert meta["live_qubits"] == 8 and meta["n_segments"] == 60 and meta["trajectory_walk"] == walk
    check_w67_counts(res.get_counts(), W67_SHOTS)


def test_w67_values_are_python_ints_and_narrow_registers_stay_uint64():
    vals, cnts, nclb, _, _ = trajectory.run_trajectories(w67_circuit(), 200, 3, engine_factory=br.factory, walk="levels")
    assert nclb == 67 and vals.dtype == object and all(isinstance(v, int) for v in vals) and cnts.sum() == 200
    assert max(vals).bit_length() > 64
    vals, cnts, nclb, _, _ = trajectory.run_trajectories(QCMRF([[0, 1], [1, 2]], random_theta(8)), 200, 3,
                                                        engine_factory=br.factory, walk="levels")
    assert nclb == 6 and vals.dtype == np.uint64


@pytest.mark.parametrize("fusion", [0, 3])
def test_levels_counts_follow_the_closed_form(models, fusion):
    for j in (2, 5):
        C = models["0.5"]["GRAPHS"][j]
        th = models["0.5"]["THETAS"][str(j)][3]
        shots = 60000
        vals, cnts, nclb, cregs, meta = trajectory.run_trajectories(QCMRF(C, th), shots, 11, fusion=fusion,
                                                                    engine_factory=br.factory, walk="levels")
        n, m, W, dim = cf.model_shape(C)
        assert meta["live_qubits"] == n + 2 and nclb == W and cnts.sum() == shots
        p = cf.probabilities(C, th)
        obs = np.zeros(p.size)
        for v, c in zip(vals.tolist(), cnts.tolist()):
            obs[v] += c
        assert obs[p == 0].sum() == 0
        sel = p * shots > 5
        chi = ((obs[sel] - p[sel] * shots) ** 2 / (p[sel] * shots)).sum() / (sel.sum() - 1)
        assert 0.8 < chi < 1.25


@pytest.mark.parametrize("slots", [1, 2, 64])
def test_exact_replay_of_the_binomial_draws(slots):
    C = workloads.chain(6)
    qc = QCMRF(C, random_theta(20))
    shots, seed = 3000, 17
    segs = trajectory.compile_trajectory(qc)[0]
    runs = []
    for _ in range(2):
        trace = []
        vals, cnts, _, _, meta = trajectory.run_trajectories(qc, shots, seed, engine_factory=br.factory, walk="levels",
                                                             slots=slots, trace=trace)
        runs.append((vals.tolist(), cnts.tolist(), trace, meta["branch_nodes"], meta["batches"]))
    assert runs[0] == runs[1]                                  # run after run: the same draws, the same counts
    vals, cnts, trace, nodes, batches = runs[0]
    assert sum(cnts) == shots and meta["trajectory_slots"] == slots and batches == len(trace)
    assert max(len(t[1]) for t in trace) == meta["max_batch_slots"] <= slots
    n_leaves = br.replay_draws(trace, seed, len(segs) - 1)
    per_level = br.check_tree(trace, segs, shots)
    assert nodes == sum(per_level.values()) + n_leaves
    if slots == 1:
        assert all(len(t[1]) == 1 for t in trace)


@pytest.mark.parametrize("seed", [17, 5, 3])
def test_one_slot_per_batch_walks_the_tree_of_the_depth_walk(seed):
    """slots = 1: one branch per batch, and the draws fall in the order of the depth walk -- the same number of nodes (and,
    on this engine, the same counts).  chain(12) with 150 shots: 10 mid-circuit measurements, far fewer shots than the 2^10
    paths, so the tree is what the draws make it, not the full one"""
    qc = QCMRF(workloads.chain(12), random_theta(44, 0.25))
    shots = 150
    d = trajectory.run_trajectories(qc, shots, seed, engine_factory=br.factory)
    l = trajectory.run_trajectories(qc, shots, seed, engine_factory=br.factory, walk="levels", slots=1)
    assert d[4]["n_segments"] == 11 and 11 < d[4]["branch_nodes"] < 2 ** 11 - 1
    assert l[4]["branch_nodes"] == d[4]["branch_nodes"]
    assert l[4]["max_batch_slots"] == 1
    assert dict(zip(l[0].tolist(), l[1].tolist())) == dict(zip(d[0].tolist(), d[1].tolist()))


def test_other_slots_other_draws_same_distribution():
    qc = QCMRF(workloads.chain(6), random_theta(20))
    a = trajectory.run_trajectories(qc, 3000, 17, engine_factory=br.factory, walk="levels", slots=1)
    b = trajectory.run_trajectories(qc, 3000, 17, engine_factory=br.factory, walk="levels", slots=64)
    assert a[1].sum() == b[1].sum() == 3000 and a[4]["batches"] > b[4]["batches"]


class CountingFactory:
    """engines of the reference kind; counts the amplitudes allocated and not yet closed"""

    def __init__(self):
        self.alive = self.peak = 0

    def __call__(self, n, devices=(0,), **kw):
        outer = self

        class Eng(br.BranchNumpyEngine):
            def close(self):
                if not getattr(self, "_closed", False):
                    self._closed = True
                    outer.alive -= 1 << self.n_qubits

        self.alive += 1 << n
        self.peak = max(self.peak, self.alive)
        return Eng(n, 1)


@pytest.mark.parametrize("slots", [1, 4, 64])
def test_memory_rule(slots):
    qc = QCMRF(workloads.chain(6), random_theta(20))
    segs, width = trajectory.compile_trajectory(qc)[:2]
    f = CountingFactory()
    meta = trajectory.run_trajectories(qc, 3000, 5, engine_factory=f, walk="levels", slots=slots)[4]
    assert f.alive == 0                                        # every engine closed at the end
    assert 0 < f.peak <= (len(segs) + 2) * slots * 2 ** width
    if slots == 64:
        # every level fits one run: its source goes back to the pool before the walk descends, so no more than the batch
        # and the engine being filled from it (or a leaf's) are ever in use
        assert meta["max_batch_slots"] <= slots and meta["max_engines_in_use"] == 2
    if slots == 1:
        assert meta["max_engines_in_use"] > 2                  # a source waits for its second run


def test_explicit_slots_that_cannot_fit_are_a_memory_error():
    qc = QCMRF(workloads.chain(6), random_theta(20))
    f = CountingFactory()
    f.free_bytes = 1 << 20
    with pytest.raises(MemoryError, match="bytes"):
        trajectory.run_trajectories(qc, 100, 5, engine_factory=f, walk="levels", slots=1 << 12)
    assert f.peak == 0                                         # before any work is done
    meta = trajectory.run_trajectories(qc, 100, 5, engine_factory=f, walk="levels")[4]
    segs, width = trajectory.compile_trajectory(qc)[:2]
    s = meta["trajectory_slots"]
    assert s >= 1 and (len(segs) + 2) * s * (16 << width) <= 0.8 * f.free_bytes < (len(segs) + 2) * 2 * s * (16 << width)
    assert trajectory.default_slots(8) == 1 << 18 and trajectory.default_slots(30) == 1


def test_depth_walk_is_unchanged():
    """vals / cnts of the depth walk at <= 64 classical bits, recorded from the commit before the levels walk existed"""
    cases = json.load(open(os.path.join(GOLDEN, "trajectory_depth_walk.json")))
    assert len(cases) == 3
    for c in cases:
        vals, cnts, _, _, meta = trajectory.run_trajectories(QCMRF(c["cliques"], c["theta"]), c["shots"], c["seed"],
                                                             fusion=c["fusion"], engine_factory=br.factory)
        assert vals.dtype == np.uint64 and cnts.dtype == np.int64 and meta["trajectory_walk"] == "depth"
        assert vals.tolist() == c["vals"] and cnts.tolist() == c["cnts"] and meta["branch_nodes"] == c["branch_nodes"], c["name"]


def test_refusals():
    from qcmrf_amd.noise import NoiseModel, depolarizing_error
    qc = QCMRF([[0, 1], [1, 2]], random_theta(8))
    be = QsvBackend(method="trajectory")
    be._engine_factory = br.factory
    with pytest.raises(ValueError, match="walk"):
        be.run(qc, shots=10, trajectory_walk="breadth")
    with pytest.raises(ValueError, match="walk"):
        trajectory.run_trajectories(qc, 10, 1, engine_factory=br.factory, walk="breadth")
    for bad in (3, 0, -2, 6, 2.5):
        with pytest.raises(ValueError, match="power of two"):
            be.run(qc, shots=10, trajectory_walk="levels", trajectory_slots=bad)
    with pytest.raises(ValueError, match="levels"):
        be.run(qc, shots=10, trajectory_slots=4)               # the depth walk has no slots
    for walk in ({}, {"trajectory_walk": "depth"}):
        with pytest.raises(ValueError, match="trajectory_trace"):
            be.run(qc, shots=10, trajectory_trace=[], **walk)  # the depth walk has no batches to record
    sv = QsvBackend()
    sv._engine_factory = br.factory
    for opt in ({"trajectory_walk": "levels"}, {"trajectory_walk": "depth"}, {"trajectory_slots": 4}, {"trajectory_trace": []}):
        with pytest.raises(ValueError, match="method='trajectory'"):
            sv.run(qc, shots=10, **opt)
    nm = NoiseModel()
    nm.add_all_qubit_quantum_error(depolarizing_error(0.01, 1), ["sx", "x", "id"])
    for walk in ("depth", "levels"):
        with pytest.raises(ValueError, match="trajectory"):
            be.run(qc, shots=10, noise_model=nm, trajectory_walk=walk)
