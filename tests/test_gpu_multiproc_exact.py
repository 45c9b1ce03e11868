"""GPU: 2 and 4 libqsv ranks as separate processes on device 0, held to exact references (_gpu_rank_exact_worker.py).

  exchange   the peer-mapped transport of exchange_multi -- k_swap_blocks over half ranges between ipc_group_barriers --
             on the whole table of _exchange_cases.py: both forms of the kernel, one-block shards where the lower rank of
             a pair moves nothing, twelve exchanges with changing peer groups, a gate right behind an exchange
  sampling   the merged count dict of a multi-rank run(), rebuilt from the split, the rank seeds and every rank's words;
             the words themselves against the inverse-CDF reference; expectation_diagonal summed over the ranks

The ranks are plain processes with the launcher's variables in their environment, as test_multiproc_gloo.py starts its
socket workers.  The parent waits on all of them; the first rank that fails, or a limit far below the 120 s the ranks'
own barrier waits, ends the others, and the test fails with what every rank printed.  Nothing is tried twice."""
import json
import os
import socket
import subprocess
import sys
import time

import pytest

import _exchange_cases as xc
from conftest import ROOT

pytestmark = pytest.mark.gpu

LIMIT_S = {"exchange": 40.0, "sampling": 60.0}      # a launch takes 0.5 s and 2 s (profiles/multirank_exact.log); the ranks' barrier gives up at 120 s


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _tail(path, n=3000):
    with open(path, "rb") as f:
        f.seek(0, os.SEEK_END)
        f.seek(max(0, f.tell() - n))
        return f.read().decode("utf-8", "replace")


def launch(world, part, tmp_path):
    """run the worker on ``world`` ranks; the per-rank results, or a failure that quotes every rank's output"""
    assert world <= 4
    port = free_port()
    out = str(tmp_path / "result")
    procs, logs = [], []
    for r in range(world):
        env = dict(os.environ, OMP_NUM_THREADS="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(r),
                   WORLD_SIZE=str(world), LOCAL_RANK=str(r), LOCAL_WORLD_SIZE=str(world), HSA_ENABLE_IPC_MODE_LEGACY="0")
        logs.append(str(tmp_path / ("rank%d.log" % r)))
        with open(logs[-1], "wb") as log:
            procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_gpu_rank_exact_worker.py"), part, out],
                                          cwd=ROOT, env=env, stdout=log, stderr=subprocess.STDOUT))
    deadline = time.monotonic() + LIMIT_S[part]
    verdict = None
    try:
        while verdict is None:
            running = [p for p in procs if p.poll() is None]
            codes = [p.returncode for p in procs if p.returncode is not None]
            if any(codes):
                verdict = "rank exited with %s" % [p.returncode for p in procs]
            elif not running:
                verdict = "ok"
            elif time.monotonic() > deadline:
                verdict = "not finished after %.0f s (still running: ranks %s)" % (LIMIT_S[part], [procs.index(p) for p in running])
            else:
                try:
                    running[0].wait(timeout=min(0.25, max(0.01, deadline - time.monotonic())))
                except subprocess.TimeoutExpired:
                    pass
    finally:
        for p in procs:                    # whatever happened: no rank outlives the test
            if p.poll() is None:
                p.kill()
        for p in procs:
            p.wait()
    if verdict != "ok":
        pytest.fail("%d ranks, %s: %s\n%s" % (world, part, verdict, "\n".join("--- rank %d ---\n%s" % (r, _tail(l)) for r, l in enumerate(logs))))
    res = [json.load(open("%s.rank%d.json" % (out, r))) for r in range(world)]
    for r, v in enumerate(res):
        assert v["rank"] == r and v["world"] == world and v["bad"] == [], v["bad"][:10]
    return res


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.timeout(120)
def test_exchange_between_rank_processes(tmp_path, world):
    res = launch(world, "exchange", tmp_path)
    cases = [c for c in xc.all_cases() if c.P == world]
    seqs = {n: s for n, s in xc.SEQUENCES.items() if s[1] == world}
    want = {"%s/%d" % (c.name, swz): c.exchanges for c in cases for swz in (0, 2)}
    for n in seqs:
        counts = xc.sequence_exchanges(n)
        want.update({"%s/%d/%d" % (n, k, swz): sum(counts[:k + 1]) for k in range(len(counts)) for swz in (0, 2)})
    for v in res:
        assert v["exchanges"] == want                       # every case ran, the same count on every rank, the table's
        assert v["compared"] == len(want)
    assert any(c.swizzled for c in cases) and any(not c.swizzled and c.exchanges for c in cases)
    assert any(c in xc.small_cases() for c in cases)        # the one-block shards went through the IPC export too


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.timeout(150)
def test_counts_of_a_multi_rank_run(tmp_path, world):
    res = launch(world, "sampling", tmp_path)
    for v in res:
        assert set(v["runs"]) == set(xc.RUNS)
    for name, run in xc.RUNS.items():
        rows = [v["runs"][name] for v in res]
        assert all(r["split"] == rows[0]["split"] for r in rows) and sum(rows[0]["split"]) == xc.SHOTS, (name, rows)
        assert [r["shots"] for r in rows] == rows[0]["split"], (name, rows)
        assert all(r["exchanges"] == rows[0]["exchanges"] for r in rows), (name, rows)
        index = xc.expects_index_order(run, [o.kind for o in xc.plan_of(name, world).ops])
        for r in rows:
            assert r["err"] < 1e-12 and r["expect_err"] < 1e-13, (name, r)
            assert r["path"] == (None if r["shots"] == 0 else "index" if index else "tile"), (name, r)
    by = {name: [v["runs"][name] for v in res] for name in xc.RUNS}
    assert 0 in by["sparse_reference_empty_ranks"][0]["split"]                       # a rank without shots drew nothing
    assert by["chain8_reference_fused"][0]["exchanges"] == 1 and by["chain8_auto_sweeps"][0]["exchanges"] == 0
    assert "sparse_auto_index_order" in res[0].get("merged_duplicates", [])         # two ranks drew the same outcome: the merge added
