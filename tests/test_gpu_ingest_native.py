"""Runs on the device with the native block reader on and off: identical counts for one seed, identical state vector,
and the run's metadata says which path read the blocks."""
import json
import os

import numpy as np
import pytest

from qcmrf_amd import QCMRF, workloads
from qcmrf_amd import ingest as ing_mod
from qcmrf_amd.backend import QsvBackend

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _cases():
    g = json.load(open(os.path.join(HERE, "golden", "config1.json")))
    chain = workloads.chain(9)
    return {"config1": (g["cliques"], g["theta"], 8),
            "chain9": (chain, workloads.theta_halfnorm(workloads.dimension(chain)), 18)}


@pytest.fixture(scope="module")
def backend():
    be = QsvBackend()
    yield be
    be.close()


@pytest.mark.parametrize("name", ["config1", "chain9"])
def test_runs_agree_with_the_native_reader_on_and_off(backend, name):
    assert ing_mod.native_available(), "qcmrf_amd._ingest_native is not built (python -m qcmrf_amd.build)"
    cliques, theta, width = _cases()[name]
    qc = QCMRF(cliques, theta)
    assert qc.num_qubits == width
    got = {}
    was = ing_mod.use_native(True)
    assert was is True                                   # the default where the module imports
    try:
        for on in (True, False):
            ing_mod.use_native(on)
            res = backend.run(qc, shots=2048, seed_simulator=1984).result()
            got[on] = (res.get_counts(), res.metadata(0)["ingest_path"], np.array(backend.statevector(), copy=True))
    finally:
        ing_mod.use_native(was)
    assert got[True][1] == "native" and got[False][1] == "python"
    assert sum(got[True][0].values()) == 2048
    assert got[True][0] == got[False][0]
    assert got[True][2].shape == (1 << width,) and got[True][2].tobytes() == got[False][2].tobytes()
