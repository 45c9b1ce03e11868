"""Runs on the device with the native back half of the front end (``frontend.build_program``) on and off: the same counts
dict in the same order, the same state vector byte for byte, and the run's metadata says which path planned and encoded the
program.  No kernel is involved in the change, so these are end-to-end equalities at the smallest shapes."""
import numpy as np
import pytest

from qcmrf_amd import QCMRF, workloads
from qcmrf_amd import ingest as ing_mod
from qcmrf_amd.backend import QsvBackend

import _frontend_cases as fc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def backend():
    be = QsvBackend()
    yield be
    be.close()


@pytest.fixture(autouse=True)
def _switches_on():
    assert ing_mod.native_available(), "qcmrf_amd._ingest_native is not built (python -m qcmrf_amd.build)"
    assert ing_mod.use_native(True) is True and ing_mod.use_native_frontend(True) is True and ing_mod.use_native_program(True) is True
    yield
    ing_mod.use_native_program(True)


def _circuit(name):
    if name == "baseline1":                                  # BASELINE configs[1]: the chain of 10 variables, W = 20
        c = workloads.baseline_config(1)[1]
        return QCMRF(c, fc.theta(c))
    return fc.accepted(name)


def _both(backend, qc, shots, **options):
    got = {}
    for on in (True, False):
        ing_mod.use_native_program(on)
        res = backend.run(qc, shots=shots, seed_simulator=1984, **options).result()
        got[on] = (res.get_counts(), res.metadata(0), np.array(backend.statevector(), copy=True), len(backend.last_plan.ops))
    ing_mod.use_native_program(True)
    return got


@pytest.mark.parametrize("name,width,shots,devices", [("vertex", 3, 512, 1), ("edge", 4, 512, 1), ("triangle", 5, 512, 1),
                                                      ("chain9", 18, 512, 1), ("config1", 8, 2048, 1), ("baseline1", 20, 2048, 1),
                                                      ("triangle", 5, 512, 2)])
def test_runs_agree_with_the_native_program_on_and_off(backend, name, width, shots, devices):
    qc = _circuit(name)
    assert qc.num_qubits == width
    got = _both(backend, qc, shots, devices=(0,) * devices)
    assert got[True][1]["plan_path"] == "native" and got[False][1]["plan_path"] == "python"
    assert got[True][1]["compile_path"] == got[False][1]["compile_path"] == "blocks"
    for key in ("n_source_ops", "n_device_ops", "layout", "n_qubits", "n_shards", "n_exchanges"):
        assert got[True][1][key] == got[False][1][key], key
    assert got[True][1]["n_shards"] == devices and got[True][1]["n_device_ops"] == got[True][3] == got[False][3]
    assert sum(got[True][0].values()) == shots
    assert got[True][0] == got[False][0] and list(got[True][0]) == list(got[False][0])
    assert got[True][2].shape == (1 << width,) and got[True][2].tobytes() == got[False][2].tobytes()


def test_post_selected_run_agrees(backend):
    qc = _circuit("chain9")
    got = _both(backend, qc, 512, post_select=qc.post_selection())
    assert got[True][1]["plan_path"] == "native" and got[False][1]["plan_path"] == "python"
    assert got[True][0] == got[False][0] and list(got[True][0]) == list(got[False][0]) and sum(got[True][0].values()) == 512
    assert got[True][1]["post_select_probability"] == got[False][1]["post_select_probability"] > 0


def test_declined_circuit_runs_as_before(backend):
    qc = fc.accepted("chain3")
    qc.global_phase = 0.3                                    # the front end takes it, the back half leaves the phase to the planner
    got = _both(backend, qc, 512)
    assert got[True][1]["plan_path"] == got[False][1]["plan_path"] == "python"
    assert got[True][1]["compile_path"] == got[False][1]["compile_path"] == "blocks"
    assert got[True][0] == got[False][0] and sum(got[True][0].values()) == 512
    assert got[True][2].tobytes() == got[False][2].tobytes()
    ref = _both(backend, fc.accepted("chain3"), 512)         # (the phase is in the state: the circuit was not taken for its neighbour)
    assert ref[True][1]["plan_path"] == "native" and ref[True][2].tobytes() != got[True][2].tobytes()
    assert np.array_equal(np.abs(ref[True][2]) > 0, np.abs(got[True][2]) > 0)
