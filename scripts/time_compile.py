"""host compile time of the 34-qubit circuit by stage (ingest, passes, plan, encode), no GPU needed, for both settings
of the ingest switch (native block reader on / off; a tree without the reader reports the Python path alone), and the
native front end that stands in for ingest + passes on the run path (qcmrf_amd/frontend.py) as a stage of its own, with its
native back half (fold + plan + encode in one call, frontend.build_program) on and off:
    python scripts/time_compile.py            in-tree circuit container
    python scripts/time_compile.py --strict   the strict Qiskit double of tests/strict_qiskit (HAVE_QISKIT branch)
    python scripts/time_compile.py --walk     also: what the top-level loop of the walk costs next to the block reads
Every AND is a distinct object either way (QCMRF.py:225,227 builds a fresh one per append)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
if "--strict" in sys.argv:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "tests", "strict_qiskit"))
import numpy as np
import qcmrf_amd
from qcmrf_amd import QCMRF, workloads, program, passes, planner
from qcmrf_amd import ingest as ing_mod
from qcmrf_amd.backend import QsvBackend
from qcmrf_amd.ingest import ingest

REPS = int(next((a.split("=")[1] for a in sys.argv if a.startswith("--reps=")), 30))
W = int(next((a.split("=")[1] for a in sys.argv if a.startswith("--w=")), 34))
name, C = workloads.baseline_config(4) if W == 34 else ("W=%d" % W, workloads.for_width(W))
th = workloads.theta_halfnorm(workloads.dimension(C))
t0 = time.perf_counter()
qc = QCMRF(C, th)
t_build = time.perf_counter() - t0
n_and, ids = 0, set()
for ci in qc.data:
    d = getattr(ci.operation, "definition", None) if ci.operation.name.startswith("cU_C") else None
    if d is not None:
        for c in d.data:
            if c.operation.name.startswith("and"):
                n_and += 1
                ids.add(id(c.operation))
be = QsvBackend()
fusion = be.options["fusion"]
print("HAVE_QISKIT=%s  %s: %d top-level instructions, %d AND instances (%d distinct objects), QCMRF() %.1f ms"
      % (qcmrf_amd.HAVE_QISKIT, name, len(qc.data), n_and, len(ids), t_build * 1e3))


def stages(reps):
    """best of ``reps`` per stage, the stages being what QsvBackend.compile and program.encode do one after the other"""
    best = {}
    for rep in range(reps):
        t0 = time.perf_counter()
        ing = ingest(qc, peephole=fusion >= 1, compact=fusion >= 3)
        t1 = time.perf_counter()
        ops = passes.optimise(ing.ops, level=fusion, fresh=True, dense_kmax=max(1, min(5, ing.num_qubits)), flat=ing.flat)
        t2 = time.perf_counter()
        pl = planner.plan(ops, ing.num_qubits, 1, be.options["layout"], lane_targets=True, dyn_lanes=planner.DYN_LANES)
        t3 = time.perf_counter()
        rec, data = program.encode(pl.ops)
        t4 = time.perf_counter()
        be.compile(qc, 1)
        t5 = time.perf_counter()
        for k, v in (("ingest", t1 - t0), ("passes", t2 - t1), ("plan", t3 - t2), ("encode", t4 - t3), ("compile()", t5 - t4)):
            best[k] = min(best.get(k, 1e9), v)
    return ing, pl, best


settings = [None]
if hasattr(ing_mod, "use_native"):
    settings = [True, False] if ing_mod.native_available() else [False]
for on in settings:
    if on is not None:
        ing_mod.use_native(on)
    ing, pl, best = stages(REPS)
    print("ingest_path=%s  device ops: %s ... total %d  source gates %d" % (getattr(ing, "ingest_path", "python (no switch in this tree)"),
          [o.kind for o in pl.ops][:6], len(pl.ops), ing.n_source_ops))
    print("  best of %d [ms]:" % REPS, {k: round(v * 1e3, 3) for k, v in best.items()})


def front_end(reps):
    """the fast path of QsvBackend._prepare by stage: the native walk alone, walk + numpy half (= ingest + passes of the other
    path), and _prepare as a whole (front end + plan + encode) with the front end on and off; where the tree has the native
    back half, also the front half alone (walk + facts + floating point), the back half alone (one multiply per table shape
    + the native call), and _prepare with the back half on and off"""
    from qcmrf_amd import frontend
    best = {}
    opts = dict(be.options)
    back = hasattr(ing_mod, "use_native_program")
    for rep in range(reps):
        t0 = time.perf_counter()
        got = frontend._describe(qc)
        t1 = time.perf_counter()
        fast = frontend.compile_blocks(qc)
        t2 = time.perf_counter()
        prepared = be._prepare(qc, opts)
        t3 = time.perf_counter()
        was = ing_mod.use_native_frontend(False)
        t4 = time.perf_counter()
        be._prepare(qc, opts)
        t5 = time.perf_counter()
        ing_mod.use_native_frontend(was)
        rows = [("read_circuit (native walk)", t1 - t0), ("compile_blocks (walk + numpy half)", t2 - t1),
                ("_prepare, front end on", t3 - t2), ("_prepare, front end off", t5 - t4)]
        if back:
            t6 = time.perf_counter()
            front = frontend.front_half(qc, 5)
            t7 = time.perf_counter()
            done = frontend.build_program(front, 1, opts["layout"])
            t8 = time.perf_counter()
            ops = frontend.fold_ops(*front[1:])
            t9 = time.perf_counter()
            was = ing_mod.use_native_program(False)
            t10 = time.perf_counter()
            slow = be._prepare(qc, opts)
            t11 = time.perf_counter()
            ing_mod.use_native_program(was)
            assert done is not None and prepared[0].plan_path == "native" and slow[0].plan_path == "python" and len(ops) == len(done[0].ops)
            rows += [("front_half (walk + facts + floating point)", t7 - t6), ("build_program (native fold + plan + encode)", t8 - t7),
                     ("fold_ops (the fold in numpy)", t9 - t8), ("_prepare, native program off (fold_ops + plan + encode)", t11 - t10)]
        for k, v in rows:
            best[k] = min(best.get(k, 1e9), v)
    assert got is not None and fast is not None and prepared[0].compile_path == "blocks"
    print("front end: compile_path=%s plan_path=%s, %d groups, %d fused ops" % (prepared[0].compile_path, getattr(prepared[0], "plan_path", "python (no switch in this tree)"),
                                                                                len(got[3]), len(fast[1])))
    print("  best of %d [ms]:" % reps, {k: round(v * 1e3, 3) for k, v in best.items()})


if hasattr(ing_mod, "use_native_frontend") and ing_mod.native_available():
    ing_mod.use_native(True)
    front_end(REPS)


def per_instruction_part():
    """the part of the top-level loop of ingest._walk that native code could take over: the tuple reads, the qi[id(b)]
    mapping and the dispatch between primitive and composite -- with no handler and no block behind it"""
    qi, _ = ing_mod._bit_maps(qc)
    qmap = list(range(qc.num_qubits))
    primitives = ing_mod._PRIMITIVES
    triples = [(ci.operation, ci.qubits, ci.clbits) for ci in qc.data]
    for op, qargs, cargs in triples:
        q = [qmap[qi[id(b)]] for b in qargs]
        name = op.name
        if getattr(op, "condition", None) is not None:
            raise ValueError(name)
        if name == "measure" or name in ("barrier", "delay") or name == "reset":
            continue
        if primitives.get(name) is None:
            getattr(op, "definition", None)


if "--walk" in sys.argv and hasattr(ing_mod, "use_native"):
    best = 1e9
    for rep in range(REPS):
        t0 = time.perf_counter()
        per_instruction_part()
        best = min(best, time.perf_counter() - t0)
    print("per-instruction part of the top-level loop alone (%d instructions): %.3f ms" % (len(qc.data), best * 1e3))
    # the walk with the block reads taken out: every composite answered from a table filled by one walk before
    for on in settings:
        ing_mod.use_native(on)
        real = ing_mod._emit_phase_block
        seen = {}

        def record(definition, qmap, out, real=real, seen=seen):
            n0, s0 = len(out.ops), out.n_source_ops
            ok = real(definition, qmap, out)
            seen[id(definition)] = (out.ops[n0:], out._phase_blocks[-1] if ok else None, out.n_source_ops - s0, ok)
            return ok

        def replay(definition, qmap, out, seen=seen):
            ops, blk, n_src, ok = seen[id(definition)]
            if ok:
                out.ops.extend(ops)
                out._phase_blocks.append(blk)
                out.n_source_ops += n_src
                out._read_by[1] += 1
            return ok

        ing_mod._emit_phase_block = record
        ingest(qc, peephole=True, compact=True)
        best_all = best_rest = 1e9
        for rep in range(REPS):
            ing_mod._emit_phase_block = real
            t0 = time.perf_counter()
            ingest(qc, peephole=True, compact=True)
            t1 = time.perf_counter()
            ing_mod._emit_phase_block = replay
            t2 = time.perf_counter()
            ingest(qc, peephole=True, compact=True)
            t3 = time.perf_counter()
            best_all, best_rest = min(best_all, t1 - t0), min(best_rest, t3 - t2)
        ing_mod._emit_phase_block = real
        print("native=%s  ingest %.3f ms, of which everything but the block reads %.3f ms (flat attempt, top-level loop, primitive "
              "handlers, one exp over all tables)" % (on, best_all * 1e3, best_rest * 1e3))
