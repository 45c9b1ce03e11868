"""Worker of tests/test_gpu_multiproc_exact.py: one libqsv rank per process, all on device 0, started as a plain process
with RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT in its environment (qcmrf_amd.comm.SocketComm; no launcher, no torch).

  exchange   every case of _exchange_cases.py whose shard count is this world size, over the peer-mapped transport:
             each rank loads its slice of the index-encoding state, the ranks call swap_layout together, each compares its
             shard with its slice of the exact permutation
  sampling   the runs of _exchange_cases.RUNS through QsvBackend(comm=...): every rank rebuilds the split, redraws its own
             shots in order and holds each word to the uniform that drew it; rank 0 rebuilds the merged dict from all words

Nothing is raised on a mismatch: a rank that left early would leave its partners waiting at a barrier.  Every finding goes
into ``bad``; the rank writes <out>.rank<r>.json and exits 1 if there is any."""
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from qcmrf_amd import _lib                           # noqa: E402
_lib.load()
assert _lib.device_count() >= 1

import _exchange_cases as xc                          # noqa: E402
from qcmrf_amd.comm import SocketComm                # noqa: E402

SWIZZLES = (0, 2)


def exchange_part(comm, bad, info):
    rank, world = comm.rank, comm.world
    shapes = sorted({(c.W, c.P) for c in xc.all_cases() if c.P == world} | {(W, P) for W, P, _ in xc.SEQUENCES.values() if P == world})
    info["exchanges"] = {}
    info["compared"] = 0
    for W, P in shapes:
        L = W - xc.log2i(P)
        lo, n = rank << L, 1 << L
        mine = slice(lo, lo + n)
        state = xc.encode_state(W)[mine]
        cases = [c for c in xc.all_cases() if (c.W, c.P) == (W, P)]
        seqs = sorted(name for name, (w, p, _) in xc.SEQUENCES.items() if (w, p) == (W, P))
        with _lib.Engine(W, devices=(0,), rank=rank, world_size=world) as eng:
            assert eng.comm_bootstrap(comm, device=0, transport="p2p") == "p2p"
            seen = {}
            for swz in SWIZZLES:
                eng.set_option("swizzle", swz)
                for c in cases:
                    eng.set_amplitudes(lo, state)
                    eng.reset_stats()
                    eng.swap_layout(c.a, c.b)
                    got = eng.amplitudes(lo, n)
                    want = xc.expected_state(c.name)[mine]
                    if not np.array_equal(got, want):
                        bad.append("%s swizzle %d rank %d: %s" % (c.name, swz, rank, xc.first_mismatch(got, want, lo)))
                    x = eng.stats()["exchanges"]
                    if x != c.exchanges:
                        bad.append("%s swizzle %d rank %d: %d exchanges counted, %d expected" % (c.name, swz, rank, x, c.exchanges))
                    info["exchanges"]["%s/%d" % (c.name, swz)] = x
                    seen[c.name, swz] = got
                    info["compared"] += 1
                for name in seqs:
                    steps, want, counts = xc.SEQUENCES[name][2], xc.sequence_states(name), xc.sequence_exchanges(name)
                    eng.set_amplitudes(lo, state)
                    eng.reset_stats()
                    for k, st in enumerate(steps):
                        if st[0] == "swap":
                            eng.swap_layout(st[1], st[2])
                        else:
                            eng.apply_1q(st[1], st[2])
                        got = eng.amplitudes(lo, n)
                        if not np.array_equal(got, want[k][mine]):
                            bad.append("%s step %d swizzle %d rank %d: %s" % (name, k, swz, rank, xc.first_mismatch(got, want[k][mine], lo)))
                        x = eng.stats()["exchanges"]
                        if x != sum(counts[:k + 1]):
                            bad.append("%s step %d swizzle %d rank %d: %d exchanges counted, %d expected" % (name, k, swz, rank, x, sum(counts[:k + 1])))
                        info["exchanges"]["%s/%d/%d" % (name, k, swz)] = x
                        seen[name, k, swz] = got
                        info["compared"] += 1
            for key in [k for k in seen if k[-1] == 0]:
                if seen[key].tobytes() != seen[key[:-1] + (2,)].tobytes():
                    bad.append("%r rank %d: the two swizzle settings differ in bits" % (key[:-1], rank))
            comm.barrier()                            # no rank frees a shard that a partner's last step may still address


def _expectation_cases(layout, L):
    shard_q = [q for q in range(xc.WIDTH) if layout[q] >= L]
    local_q = [q for q in range(xc.WIDTH) if layout[q] < L]
    return [([shard_q[0], local_q[3], local_q[7]], {local_q[1]: 1}),
            ([local_q[0], local_q[5]], {shard_q[-1]: 0, local_q[2]: 0}),
            ([local_q[9], local_q[4], local_q[11]], {shard_q[-1]: 1}),
            (shard_q + [local_q[2]], None)]


def sampling_part(comm, bad, info):
    from _sampler_reference import TOL_REL, check_inverse_cdf, exact_index_order, sorted_uniforms, unshuffle
    from qcmrf_amd.backend import QsvBackend
    rank, world = comm.rank, comm.world
    L = xc.WIDTH - xc.log2i(world)
    lo, n = rank << L, 1 << L
    info["runs"] = {}
    be = QsvBackend(comm=comm, device=0)

    def check(ok, *what):
        if not ok:
            bad.append("rank %d: %s" % (rank, " ".join(str(w) for w in what)))

    for name in sorted(xc.RUNS):
        run = xc.RUNS[name]
        qc, amp, measured = xc.circuit_of(run.circuit)
        seed = run.seeds[world]
        res = be.run(qc, shots=xc.SHOTS, seed_simulator=seed, **xc.run_options(run)).result()
        eng, meta = be.last_engine, res.metadata(0)
        layout = meta["layout"]
        stats = eng.stats()                           # of the run itself: its passes, its norm, its draw
        prob = stats["kinds"].get("prob", {}).get("launches", 0)
        total = eng.norm()
        masses = comm.allgather_f64(total)
        split = xc.shot_split(seed, xc.SHOTS, masses)
        k = int(split[rank])
        rseed = xc.rank_seed(seed, rank)
        words = eng.sample(k, rseed) if k else np.zeros(0, dtype=np.uint64)
        shard = eng.amplitudes(lo, n)
        want = amp[xc.logical_of_physical(layout, lo, n)]
        err = float(np.abs(shard - want).max())
        check(err < 1e-12, name, "shard off the closed form by", err)
        check(stats["exchanges"] == meta["n_exchanges"], name, "exchanges", stats["exchanges"], meta["n_exchanges"])
        p = xc.probs(shard)
        path = None
        if k:
            tol = TOL_REL * total
            check(abs(total - math.fsum(p.tolist())) <= 2.5e-13 * total, name, "norm", total)
            check(bool((words >> np.uint64(L) == np.uint64(rank)).all()), name, "words outside this rank's shard")
            r = sorted_uniforms(rseed, k, total)
            x = unshuffle(rseed, k, words) - np.uint64(lo)
            broken = check_inverse_cdf(p, r, x, tol, total)
            check(broken == [], name, "contract", broken)
            path = "index" if prob > 0 else "tile"
            check((prob > 0) == xc.expects_index_order(run, [o.kind for o in be.last_plan.ops]), name, "path", path, "prob launches", prob)
            if prob > 0:
                wantx, dist = exact_index_order(p, r)
                check(int((dist <= tol).sum()) == 0, name, "ambiguous uniforms", int((dist <= tol).sum()))
                miss = np.flatnonzero(x != wantx)
                check(miss.size == 0, name, "words", miss.size, miss[:5].tolist(), x[miss[:5]].tolist(), wantx[miss[:5]].tolist())
        else:
            check(total == 0.0 and not shard.any(), name, "no shots for a populated shard", total)
        everyone = comm.allgather(words)
        counts = res.get_counts()
        dicts = comm.allgather(counts)
        if rank == 0:
            expected = xc.counts_dict(xc.clbit_values(np.concatenate(everyone), layout, measured), qc.num_clbits)
            check(counts == expected, name, "merged counts differ:", len(counts), "keys against", len(expected),
                  sorted(set(counts.items()) ^ set(expected.items()))[:6])
            check(sum(counts.values()) == xc.SHOTS, name, "shots counted", sum(counts.values()))
            for r_, d in enumerate(dicts[1:], 1):
                check(d == (expected if run.gather == "all" else {}), name, "counts on rank", r_, len(d))
            per_rank = [np.unique(xc.clbit_values(ws, layout, measured)) for ws in everyone]
            if np.unique(np.concatenate(per_rank)).size < sum(u.size for u in per_rank):
                info.setdefault("merged_duplicates", []).append(name)       # an outcome that two ranks drew: the merge had to add
        exp_err = 0.0
        rs = np.random.RandomState(17)
        pl = xc.probs(amp)
        idx = np.arange(pl.size, dtype=np.int64)
        for qubits, fixed in _expectation_cases(layout, L):
            tab = rs.randn(1 << len(qubits))
            j = np.zeros_like(idx)
            for b, q in enumerate(qubits):
                j |= ((idx >> q) & 1) << b
            sel = np.ones(idx.size, dtype=bool)
            for q, v in (fixed or {}).items():
                sel &= ((idx >> q) & 1) == v
            s0, s1 = be.expectation_diagonal(tab, qubits, fixed)
            e0, e1 = abs(s0 - float((pl[sel] * tab[j[sel]]).sum())), abs(s1 - float(pl[sel].sum()))
            exp_err = max(exp_err, e0, e1)
            check(e0 < 1e-13 and e1 < 1e-13, name, "expectation_diagonal", qubits, fixed, e0, e1)
        info["runs"][name] = {"path": path, "shots": k, "split": [int(s) for s in split], "err": err, "prob": int(prob),
                              "exchanges": int(stats["exchanges"]), "layout": [int(x) for x in layout], "expect_err": exp_err}
        comm.barrier()
    be.close()


def main():
    part, out = sys.argv[1], sys.argv[2]
    comm = SocketComm(timeout_s=60)
    bad, info = [], {"rank": comm.rank, "world": comm.world, "part": part}
    {"exchange": exchange_part, "sampling": sampling_part}[part](comm, bad, info)
    info["bad"] = bad
    with open("%s.rank%d.json" % (out, comm.rank), "w") as f:
        json.dump(info, f)
    comm.barrier()
    assert "torch" not in sys.modules
    comm.close()
    for line in bad[:40]:
        print(line)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
