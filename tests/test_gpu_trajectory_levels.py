"""The level-wise walk of the trajectory mode through run() on the MI355X: qsv_exec on the wide batch, qsv_branch_mass,
qsv_branch_split, the leaves through qsv_sample."""
import numpy as np
import pytest

import _branch_reference as br
from conftest import random_theta
from oracle import closed_form as cf
from test_trajectory_levels import W67_SHOTS, check_w67_counts, w67_circuit

pytestmark = pytest.mark.gpu


def test_small_graph_follows_the_closed_form(models):
    from qcmrf_amd import QCMRF
    from qcmrf_amd.backend import QsvBackend
    tb = QsvBackend(method="trajectory", trajectory_walk="levels")
    C = models["0.5"]["GRAPHS"][3]
    th = models["0.5"]["THETAS"]["3"][1]
    shots = 50000
    res = tb.run(QCMRF(C, th), shots=shots, seed_simulator=3).result()
    counts = res.get_counts()
    n, m, W, dim = cf.model_shape(C)
    meta = res.metadata(0)
    assert meta["live_qubits"] == n + 2 and meta["trajectory_walk"] == "levels" and sum(counts.values()) == shots
    assert meta["batches"] >= 1 and meta["max_batch_slots"] <= meta["trajectory_slots"]
    p = cf.probabilities(C, th)
    obs = np.zeros(p.size)
    for k, v in counts.items():
        obs[int(k, 2)] += v
    assert obs[p == 0].sum() == 0
    sel = p * shots > 5
    assert 0.8 < ((obs[sel] - p[sel] * shots) ** 2 / (p[sel] * shots)).sum() / (sel.sum() - 1) < 1.25
    tb.close()


def test_chain14_reproducible_and_replayed():
    """one seed, one tree: equal counts and batches run after run; the recorded draws replay exactly; every recorded
    branch probability is the reference walk's, forced along the device's outcomes, within the probability parity 1e-10"""
    from qcmrf_amd import QCMRF, trajectory, workloads
    from qcmrf_amd.backend import QsvBackend
    tb = QsvBackend(method="trajectory", trajectory_walk="levels")
    C = workloads.chain(14)
    qc = QCMRF(C, workloads.theta_halfnorm(workloads.dimension(C), scale=0.25))
    shots, seed = 2048, 1984
    traces = [[] for _ in range(3)]
    runs = [tb.run(qc, shots=shots, seed_simulator=seed, trajectory_trace=t).result() for t in traces]
    assert runs[0].get_counts() == runs[1].get_counts() == runs[2].get_counts()
    assert len({r.metadata(0)["batches"] for r in runs}) == 1 and traces[0] == traces[1] == traces[2]
    assert sum(runs[0].get_counts().values()) == shots
    assert tb.run(qc, shots=shots, seed_simulator=7).result().get_counts() != runs[0].get_counts()
    tb.close()
    trace = traces[0]
    segs, width = trajectory.compile_trajectory(qc)[:2]
    assert runs[0].metadata(0)["batches"] == len(trace)
    br.replay_draws(trace, seed, len(segs) - 1)
    br.check_tree(trace, segs, shots)
    # the reference walk along the same outcomes: states of the branches by numpy, level by level
    level_nodes = {}
    for level, bits, ks, m0, m1, k1 in trace:
        for i, b in enumerate(bits):
            level_nodes.setdefault(level, {})[b] = (m0[i], m1[i], ks[i], k1[i])
    root = br.BranchNumpyEngine(width, 1)
    states = {0: root.sh[0]}
    worst = 0.0
    for level in sorted(level_nodes):
        sg = segs[level]
        nxt = {}
        for b, (m0, m1, k, k1) in level_nodes[level].items():
            e = br.BranchNumpyEngine(width, 1)
            e.sh[0][:] = states[b]
            if len(sg.rec):
                e.exec(sg.rec, sg.data)
            want = br.mass_array(e.sh[0], width, 1, sg.measure_slot)[0]
            pw = float(want[1] / (want[0] + want[1]))
            worst = max(worst, abs(m1 / (m0 + m1) - pw))
            for o, kk in ((0, k - k1), (1, k1)):
                if kk:
                    nxt[b | (o << sg.measure_clbit)] = br.split_array(e.sh[0], 1 << width, width, [0], [o], sg.measure_slot, sg.release)
        states = nxt
    assert worst < 1e-10, worst


@pytest.mark.parametrize("slots", [None, 4])
def test_w67_on_the_device(slots):
    from qcmrf_amd.backend import QsvBackend
    tb = QsvBackend(method="trajectory")
    qc = w67_circuit()
    for walk, opt in (("levels", {"trajectory_slots": slots}), ("depth", {})):
        if walk == "depth" and slots is not None:
            continue                                          # the depth walk has no slots: run it once
        res = tb.run(qc, shots=W67_SHOTS, seed_simulator=3, trajectory_walk=walk, **opt).result()
        meta = res.metadata(0)
        assert meta["live_qubits"] == 8 and meta["n_segments"] == 60 and meta["trajectory_walk"] == walk
        if walk == "levels":
            assert meta["trajectory_slots"] == (slots or 1 << 18) and meta["max_batch_slots"] <= meta["trajectory_slots"]
        check_w67_counts(res.get_counts(), W67_SHOTS)
    tb.close()
