"""``run(..., noise_model=nm, noisy_measure=...)`` on the host: the slot plan, the records, the options, the metadata and
the refusals, with a numpy stand-in for the engine (tests/_measure_reference.py)."""
import numpy as np
import pytest

import _kraus_cases as kc
import _measure_cases as mc
from _density_matrix import chi2_pvalue
from _kraus_reference import KrausNumpyEngine
from _measure_reference import MeasureNumpyEngine, measure_density_distribution
from qcmrf_amd import QCMRF, _lib, ingest as ing_mod, trajectory
from qcmrf_amd.backend import QsvBackend


def backend(engine=MeasureNumpyEngine, **options):
    b = QsvBackend(**options)
    b._engine_factory = lambda n, devices=(0,), rank=None, world_size=None: engine(n, len(devices))
    return b


CIRCUITS = {
    "chain(4) constructed": (lambda: mc.chain_circuit(4, lowered=False), mc.constructed_model, 4),
    "chain(4) lowered": (lambda: mc.chain_circuit(4), mc.lowered_model, 4),
    "two triangles constructed": (lambda: mc.two_triangles(lowered=False), mc.constructed_model, 5),
    "two triangles lowered": (lambda: mc.two_triangles(), mc.lowered_model, 5),
    "6 variables, 20 cliques": (mc.many_cliques, mc.constructed_model, 6),
}


@pytest.mark.parametrize("name", sorted(CIRCUITS))
def test_slot_plan_and_records(name):
    make, model, n = CIRCUITS[name]
    qc, nm = make(), mc.local_readout_model(model())
    ing, rec, data, clist, meas, readout, _, state, (mode, width, n_measure) = QsvBackend._prepare_noisy(qc, nm, "auto", "in_place")
    assert (mode, width, state) == ("in_place", n + 2, "lds")
    kept = ing_mod.ingest(qc, noise=nm, keep_measures=True)
    measures = [o for o in kept.ops if o.kind == "measure"]
    trailing = 0
    while kept.ops[-1 - trailing].kind == "measure":
        trailing += 1
    mrec = rec[rec["kind"] == _lib.OP_MEASURE]
    assert n_measure == len(mrec) == len(measures) - trailing > 0
    # every mid-circuit measure is the last thing that happens to its qubit (no gate may follow a measure): all release
    assert (mrec["vals"][:, 1] == 1).all() and (mrec["n"] == 1).all()
    # the record's bit and flips are those of the LOGICAL qubit it measures
    for r, o in zip(mrec, measures):
        assert int(r["vals"][0]) == o.mask
        assert tuple(data[int(r["data_off"]):int(r["data_off"]) + 2]) == tuple(nm.readout_flips(o.target))
    # the trailing measures are one final draw; the bits written earlier are -1 there
    written = {int(c) for c in mrec["vals"][:, 0]}
    assert all(meas[c] == -1 for c in written)
    finals = {o.mask: o.target for o in measures[len(measures) - trailing:]}
    assert sorted(c for c, s in enumerate(meas) if s >= 0) == sorted(finals)
    for c, q in finals.items():
        assert tuple(readout[c]) == tuple(nm.readout_flips(q))
    # every qubit of every record is a live slot
    for r in rec:
        qs = [int(q) for q in r["qubits"][:int(r["n"])]]
        if int(r["kind"]) in (_lib.OP_1Q, _lib.OP_MCX):
            qs.append(int(r["target"]))
        assert all(0 <= q < width for q in qs)
    assert all(s < width for s in meas)
    # Pauli and Kraus ops: those of the deferred ingest, in number, order and tables
    deferred = ing_mod.ingest(qc, noise=nm)
    a = [o for o in deferred.ops if o.kind in ("pauli", "kraus")]
    b = [o for o in ing.ops if o.kind in ("pauli", "kraus")]
    assert len(a) == len(b) == deferred.n_pauli + deferred.n_kraus > 0
    assert all(x.kind == y.kind and len(x.qubits) == len(y.qubits) and np.array_equal(x.table, y.table) for x, y in zip(a, b))
    # and the unitary records between them are the deferred ones too
    assert [o.kind for o in deferred.ops] == [o.kind for o in ing.ops if o.kind != "measure"]


def test_plan_slots_recycles_the_lowest_freed_slot():
    qc = mc.chain_circuit(4, lowered=False)
    ing = ing_mod.ingest(qc, keep_measures=True)
    staged, width, finals = trajectory.plan_slots(ing.ops)
    assert width == 6 and staged[-1][0] == "ops"
    mids = [item for item in staged if item[0] == "measure"]
    assert mids and all(release for _, _, _, release, _ in mids)
    assert len({s for _, s, _, _, _ in mids}) < len(mids) or len(mids) == 1      # a slot serves more than one ancilla
    assert len(finals) + len(mids) == len(ing.measure)


@pytest.fixture(scope="module")
def chain4_run():
    qc, nm = mc.chain_circuit(4), kc.thermal_model()
    b = backend()
    res = b.run(qc, shots=2000, seed_simulator=5, noise_model=nm, noisy_measure="in_place").result()
    return qc, nm, res


def test_counts_in_place_against_the_exact_distribution(chain4_run):
    qc, nm, res = chain4_run
    ing, rec, data, clist, meas, readout, _, _, (_, width, _) = QsvBackend._prepare_noisy(qc, nm, "lds", "in_place")
    exact = measure_density_distribution(rec, data, width, meas, readout)
    p = chi2_pvalue(res.get_counts(), exact, 2000)
    print("in-place counts of the stand-in engine against the exact distribution: p = %.3g" % p)
    assert p > 1e-4


def test_metadata(chain4_run):
    qc, nm, res = chain4_run
    m = res.metadata()
    assert m["method"] == "noisy" and m["noisy_measure"] == "in_place" and m["noisy_state"] == "lds"
    assert m["n_qubits"] == 6 and m["n_circuit_qubits"] == 8 and m["n_measure_ops"] > 0
    assert m["n_kraus_ops"] > 0 and m["n_pauli_ops"] > 0 and m["readout_errors"] == 7
    d = backend().run(qc, shots=10, seed_simulator=5, noise_model=nm).result().metadata()
    assert d["noisy_measure"] == "deferred" and d["n_qubits"] == d["n_circuit_qubits"] == 8 and d["n_measure_ops"] == 0
    assert (d["n_kraus_ops"], d["n_pauli_ops"]) == (m["n_kraus_ops"], m["n_pauli_ops"])


def test_auto_runs_in_place_iff_the_state_gets_narrower():
    nm = kc.thermal_model()
    m = backend().run(mc.chain_circuit(4), shots=10, seed_simulator=1, noise_model=nm, noisy_measure="auto").result().metadata()
    assert (m["noisy_measure"], m["n_qubits"]) == ("in_place", 6)
    one = QCMRF([[0, 1]], [-0.4, -1.1, -0.2, -0.9], with_measurements=True)       # n + m + 1 = n + 2: nothing to gain
    m = backend().run(one, shots=10, seed_simulator=1, noise_model=kc.constructed_model(), noisy_measure="auto").result().metadata()
    assert (m["noisy_measure"], m["n_qubits"], m["n_measure_ops"]) == ("deferred", 4, 0)


def test_refusals():
    qc, nm = mc.chain_circuit(4, lowered=False), kc.constructed_model()
    with pytest.raises(ValueError, match="noisy_measure"):
        backend().run(qc, shots=10, noise_model=nm, noisy_measure="sometimes")
    with pytest.raises(ValueError, match="noisy_measure"):
        backend().run(qc, shots=10, noisy_measure="sometimes")                     # checked with or without a model
    with pytest.raises(ValueError, match="density_matrix"):
        backend().run(qc, shots=10, noise_model=nm, method="density_matrix", noisy_measure="in_place")
    with pytest.raises(ValueError, match="trajectory"):
        backend().run(qc, shots=10, noise_model=nm, method="trajectory", noisy_measure="in_place")
    with pytest.raises(ValueError, match="trajectory"):
        backend().run(qc, shots=10, noise_model=nm, method="trajectory")


def test_default_is_deferred_word_for_word():
    """the default hands the engine what it handed it before: no MEASURE record (an engine that knows none runs it) and,
    for a seed, the same counts as noisy_measure='deferred' spelled out"""
    qc, nm = mc.chain_circuit(4), kc.thermal_model()
    old = backend(KrausNumpyEngine).run(qc, shots=200, seed_simulator=9, noise_model=nm).result()
    new = backend().run(qc, shots=200, seed_simulator=9, noise_model=nm, noisy_measure="deferred").result()
    assert old.get_counts() == new.get_counts()
    assert old.metadata()["n_device_ops"] == new.metadata()["n_device_ops"]
    ing, rec, *_ = QsvBackend._prepare_noisy(qc, nm)
    assert not (rec["kind"] == _lib.OP_MEASURE).any()


def test_batch_passes_the_option_through():
    nm = kc.thermal_model()
    res = backend().run([mc.chain_circuit(4), mc.chain_circuit(3)], shots=20, seed_simulator=2, noise_model=nm,
                        noisy_measure="in_place").result()
    assert [res.metadata(i)["noisy_measure"] for i in (0, 1)] == ["in_place"] * 2
    assert [res.metadata(i)["n_qubits"] for i in (0, 1)] == [6, 5]


def test_many_cliques_run_only_in_place():
    qc, nm = mc.many_cliques(), kc.constructed_model()
    for state in ("lds", "hbm", "auto"):
        with pytest.raises(ValueError, match="27"):
            backend().run(qc, shots=10, noise_model=nm, noisy_state=state)
    res = backend().run(qc, shots=100, seed_simulator=3, noise_model=nm, noisy_measure="in_place", noisy_state="auto").result()
    m = res.metadata()
    assert (m["n_qubits"], m["n_circuit_qubits"], m["noisy_state"], m["n_measure_ops"]) == (8, 27, "lds", 19)
    assert sum(res.get_counts().values()) == 100


def test_encode_refuses_a_bit_beyond_63_and_bad_flips():
    from qcmrf_amd import program
    with pytest.raises(ValueError):
        program.encode([mc.measure_op(0, 64, 1, (0.0, 0.0))])
    with pytest.raises(ValueError):
        program.encode([mc.measure_op(0, 3, 1, (0.0, 1.5))])
    rec, data = program.encode([mc.measure_op(2, 5, 1, None)])
    assert (int(rec[0]["kind"]), int(rec[0]["qubits"][0]), int(rec[0]["vals"][0]), int(rec[0]["vals"][1])) == (_lib.OP_MEASURE, 2, 5, 1)
    assert data.tolist() == [0.0, 0.0]
