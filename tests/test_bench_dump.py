"""CPU: bench.py --dump-outputs writes the last step's counts and a seeded sample of the LOGICAL amplitudes,
whatever the layout and however many ranks hold the shards (numpy engine in place of the device)."""
import numpy as np
import pytest

import bench
from oracle.sharded_numpy import NumpyEngine
from qcmrf_amd import QCMRF, program, workloads
from qcmrf_amd.backend import QsvBackend
from test_host_logic import logical_amplitudes


class _Backend:
    def __init__(self, eng, plan):
        self.last_engine, self.last_plan = eng, plan


class _Comm:
    """rank r's view of an allgather in which ranks 1..P-1 have already contributed"""
    def __init__(self, rank, world, parts):
        self.rank, self.world, self.parts = rank, world, parts

    def allgather(self, obj):
        self.parts[self.rank] = obj
        return [self.parts.get(r) for r in range(self.world)]


@pytest.mark.parametrize("width,shards,layout", [(11, 1, "auto"), (16, 1, "auto"), (16, 4, "reference")])
def test_dump_outputs_is_the_logical_state_and_the_counts(tmp_path, width, shards, layout):
    C = workloads.for_width(width)
    ing, pl = QsvBackend().compile(QCMRF(C, workloads.theta_halfnorm(workloads.dimension(C))), shards, fusion=2, layout=layout)
    W = ing.num_qubits
    full = NumpyEngine(W, shards)
    program.run_stepwise(full, pl.ops)
    want = logical_amplitudes(full, pl.layout, W)
    counts = {"0" * (W - 3) + "101": 7, "1" + "0" * (W - 1): 3}
    if shards == 1:
        full.multiproc = False
        bench.dump_outputs(str(tmp_path), _Backend(full, pl), _Comm(0, 1, {}), counts)
    else:
        parts = {}
        for r in list(range(1, shards)) + [0]:                 # one process per shard; rank 0 gathers last
            eng = NumpyEngine(W, shards, owned=[r])
            eng.sh[r][:] = full.sh[r]
            eng.multiproc, eng.rank = True, r
            bench.dump_outputs(str(tmp_path), _Backend(eng, pl), _Comm(r, shards, parts), counts if r == 0 else {})
    out = {n: np.load(str(tmp_path / (n + ".npy"))) for n in ("counts_outcomes", "counts", "amplitude_index", "amplitudes")}
    assert all(a.dtype == np.float64 for a in out.values())
    idx = out["amplitude_index"].astype(np.int64)
    assert idx.size == 2 ** W if 2 ** W <= bench.DUMP_AMPLITUDES else 0 < idx.size <= bench.DUMP_AMPLITUDES
    assert np.array_equal(out["amplitudes"][:, 0] + 1j * out["amplitudes"][:, 1], want[idx])
    assert out["counts_outcomes"].tolist() == [5.0, float(2 ** (W - 1))] and out["counts"].tolist() == [7.0, 3.0]
