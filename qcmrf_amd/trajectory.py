"""Trajectory mode: take every mid-circuit measurement when it occurs and release the qubit.

The reference measures each clique's ancilla right after its block and never touches it again
(/root/reference/QCMRF.py:238-239).  Deferred to the end that costs one qubit per clique
(W = n + m + 1).  Taken when it occurs, the ancilla's slot can be recycled: the live state is only
the variables, the scratch qubit and ONE ancilla (n + 2 qubits), so MRFs with far more cliques
than any statevector of width W could hold become simulable -- at the price of following the
measurement outcomes: the engine walks the tree of outcomes depth first, splitting the shots at
every measurement by a binomial draw from the exact branch probability, and only visits branches
that still hold shots.  Everything on the device is the same hand-written HIP path (the segments
between measurements are compiled by the same exact fusion passes and run through ``qsv_exec``;
the branch probability is ``qsv_probabilities``, the collapse a one-qubit 0/1 diagonal that rides in
front of the child segment's program -- one pass, the state stays unnormalised -- the branch point
``qsv_copy_state``).  No closed-form knowledge of the circuit is used.
"""
from __future__ import annotations

import time

import numpy as np

from . import _lib, ingest as _ingest, ir, passes, planner, program


_ONE = np.array([0.0, 1.0])                               # the observable |1><1| of a measured slot


class _Segment:
    # prog[outcome]: this segment's program behind the projection of the PREVIOUS segment's measurement on ``outcome``
    # (and the X that hands a released slot back in |0>), in one record list: one pass over the state instead of three
    __slots__ = ("rec", "data", "n_ops", "measure_slot", "measure_clbit", "release", "prog")


def _live_plan(ops, n_qubits):
    """first/last use of every logical qubit; slot assignment with recycling"""
    first, last = {}, {}
    for k, op in enumerate(ops):
        qs = (op.target,) if op.kind == "measure" else op.support()
        for q in qs:
            first.setdefault(q, k)
            last[q] = k
    return first, last


def plan_slots(ops):
    """The slot plan of a gate list with "measure" ops, shared by trajectory mode and by noisy runs that measure in place.

    Every logical qubit gets a slot at its first use; a measure releases its slot iff it is the last thing that happens to
    its qubit, and the lowest freed slot is handed out again first.  Returns (staged, width, final_measures): ``staged``
    alternates ("ops", [ops remapped to slots]) and ("measure", slot, clbit, release, logical qubit) and ends with an "ops"
    entry; the trailing measures (nothing but measures after them) are taken out of it and listed as ``final_measures``
    [(slot, clbit)], to be sampled jointly from the final state; ``width`` is the number of slots in use at once."""
    first, last = _live_plan(ops, None)
    # a measure is a release point iff it is the last thing that happens to its qubit
    slot_of, free, next_slot = {}, [], 0
    width = 0
    cur = []
    final_measures = []

    def slot(q):
        nonlocal next_slot, width
        if q not in slot_of:
            if free:
                slot_of[q] = free.pop(0)
            else:
                slot_of[q] = next_slot
                next_slot += 1
            width = max(width, next_slot)
        return slot_of[q]

    def remap(op):
        lay = {q: slot(q) for q in op.support()}
        o = ir.Op(op.kind, target=lay.get(op.target), ctrls=tuple(lay[c] for c in op.ctrls), vals=op.vals,
                  qubits=tuple(lay[q] for q in op.qubits), mat=op.mat, table=op.table, mats=op.mats,
                  angle=op.angle, label=op.label)
        return o

    staged = []                                # in order: ("ops", [...]) / ("measure", slot, clbit, release, logical qubit)
    for k, op in enumerate(ops):
        if op.kind == "measure":
            s = slot(op.target)
            release = last[op.target] == k
            staged.append(("ops", cur))
            staged.append(("measure", s, op.mask, release, op.target))
            cur = []
            if release:
                del slot_of[op.target]
                free.append(s)
                free.sort()
        else:
            cur.append(remap(op))
    staged.append(("ops", cur))
    # trailing measures (nothing but measures after them) are sampled jointly from the final state
    while len(staged) >= 2 and staged[-1][0] == "ops" and not staged[-1][1] and staged[-2][0] == "measure":
        staged.pop()
        _, s, c, _, _ = staged.pop()
        final_measures.insert(0, (s, c))
    return staged, width, final_measures


def plan_slots_dynamic(ops):
    """The slot plan of a gate list read with ``ingest(dynamic=True)``: "measure", "reset" and "if" ops among the gates, qubits
    used again after a measure.  ``plan_slots`` stays what it is for every list without those.

    Every logical qubit gets a slot at its first use and the lowest freed slot is handed out again first.  A measure releases
    its slot iff it is the last thing that happens to its qubit AND it stands outside every span: inside one it may not run,
    and then the qubit is not back in |0>.  A measure followed by further use of the qubit keeps the slot (release 0).  A reset
    that is the last thing on its qubit, outside every span, frees its slot, and is dropped unless the slot is handed out
    again (its next owner has to find |0> there); nothing inside a span is dropped, so the span of an "if" op counts the same
    ops before and after.  Returns (items, width, final_measures): ``items`` is the flat
    stream in order -- ir.Op remapped to slots ("if" ops copied, their span in ``target``), ("measure", slot, clbit, release,
    logical qubit) and ("reset", slot) --, the trailing measures outside every span are taken out of it and listed as
    ``final_measures`` [(slot, clbit)], to be sampled jointly from the final state; ``width`` is the number of slots in use
    at once."""
    last = {}
    for k, op in enumerate(ops):
        for q in ((op.target,) if op.kind in ("measure", "reset") else () if op.kind == "if" else op.support()):
            last[q] = k
    slot_of, free, next_slot, width = {}, [], 0, 0

    droppable = {}                             # slot -> index in items of the trailing reset that freed it, while nobody took it

    def slot(q):
        nonlocal next_slot, width
        if q not in slot_of:
            if free:
                slot_of[q] = free.pop(0)
                droppable.pop(slot_of[q], None)    # handed out again: that reset has to run
            else:
                slot_of[q] = next_slot
                next_slot += 1
            width = max(width, next_slot)
        return slot_of[q]

    def give_back(q):
        free.append(slot_of.pop(q))
        free.sort()

    items, guarded = [], []                    # guarded[i]: items[i] lies in the span of an "if" op
    span_end = 0
    for k, op in enumerate(ops):
        inside = k < span_end
        if op.kind == "if":
            if inside:
                raise ValueError("an 'if' op inside the span of another: nested conditions are not supported")
            if op.target < 1 or k + op.target > len(ops) - 1:
                raise ValueError("an 'if' op guards %d ops, %d follow it" % (op.target, len(ops) - 1 - k))
            span_end = k + 1 + op.target
            items.append(ir.Op("if", target=op.target, mask=op.mask, a=op.a, vals=op.vals))
        elif op.kind == "measure":
            release = last[op.target] == k and not inside
            items.append(("measure", slot(op.target), op.mask, release, op.target))
            if release:
                give_back(op.target)
        elif op.kind == "reset":
            if last[op.target] == k and not inside:
                if op.target not in slot_of:
                    continue                       # the qubit was never touched: nothing to reset, no slot to free
                droppable[slot_of[op.target]] = len(items)
                items.append(("reset", slot_of[op.target]))
                give_back(op.target)
            else:
                items.append(("reset", slot(op.target)))
        else:
            lay = {q: slot(q) for q in op.support()}
            items.append(ir.Op(op.kind, target=lay.get(op.target), ctrls=tuple(lay[c] for c in op.ctrls), vals=op.vals,
                               qubits=tuple(lay[q] for q in op.qubits), mat=op.mat, table=op.table, mats=op.mats,
                               angle=op.angle, label=op.label))
        guarded.append(inside)
    drop = set(droppable.values())                 # outside every span, so no span changes
    items, guarded = [x for i, x in enumerate(items) if i not in drop], [g for i, g in enumerate(guarded) if i not in drop]
    final_measures = []
    while items and isinstance(items[-1], tuple) and items[-1][0] == "measure" and not guarded[len(items) - 1]:
        _, s, c, _, _ = items.pop()
        final_measures.insert(0, (s, c))
    return items, width, final_measures


def compile_trajectory(circuit, fusion=3):
    """-> (segments, width, final_measures [(slot, clbit)], num_clbits, creg_sizes, n_source_ops)"""
    ing = _ingest.ingest(circuit, peephole=fusion >= 1, keep_measures=True)
    staged, width, final_measures = plan_slots(ing.ops)
    # fuse every segment with the ordinary exact passes (no init folding after the first one)
    segs = []
    first_seg = True
    i = 0
    while i < len(staged):
        kind = staged[i][0]
        assert kind == "ops"
        body = staged[i][1]
        if first_seg:
            fused = passes.optimise(body, level=fusion) if fusion > 0 else [ir.op_init(0)] + body
        else:
            fused = passes._fuse_body([ir.op_init(0)] + body, fusion, 10, 8)[1:] if fusion > 0 else list(body)
        first_seg = False
        sg = _Segment()
        sg.rec, sg.data = program.encode(fused)
        sg.n_ops = len(fused)
        sg.measure_slot = sg.measure_clbit = None
        sg.release = False
        sg.prog = None
        if segs:
            # the state stays UNNORMALISED along a branch (the projection is the 0/1 table, not 1/sqrt(p)): branch
            # probabilities are ratios and the sampler divides by the mass it finds
            prev = segs[-1]
            sg.prog = {}
            for outcome in (0, 1):
                pre = [ir.op_diag([prev.measure_slot], [1.0 - outcome, float(outcome)])]
                if outcome == 1 and prev.release:
                    pre.append(ir.op_x(prev.measure_slot))
                sg.prog[outcome] = program.encode(pre + list(fused))
        if i + 1 < len(staged):
            _, s, c, rel, _ = staged[i + 1]
            sg.measure_slot, sg.measure_clbit, sg.release = s, c, rel
        segs.append(sg)
        i += 2
    return segs, max(width, 1), final_measures, ing.num_clbits, ing.creg_sizes, ing.n_source_ops


def _leaf_values(bits, smp, final_measures, wide):
    """the register values of a leaf's shots -> (sorted distinct values, their counts); ``bits`` is the Python int the
    branch has written so far, ``smp`` the sampled words (bit j = final_measures[j])"""
    if not wide:
        vals = np.full(len(smp), bits, dtype=np.uint64)
        for j, (_, c) in enumerate(final_measures):
            vals |= ((smp >> np.uint64(j)) & np.uint64(1)) << np.uint64(c)
        uv, uc = np.unique(vals, return_counts=True)
        return uv.tolist(), uc.tolist()
    agg = {}                                                # registers past 64 bits: Python ints, one per distinct word
    us, uc = np.unique(smp, return_counts=True)
    for s, c in zip(us.tolist(), uc.tolist()):
        v = bits
        for j, (_, cb) in enumerate(final_measures):
            v |= ((s >> j) & 1) << cb
        agg[v] = agg.get(v, 0) + c
    keys = sorted(agg)
    return keys, [agg[v] for v in keys]


def default_slots(width):
    """the largest power of two of slots of 2^width amplitudes within 2^30 bytes, at least 1"""
    return max(1, (1 << 30) // (16 << width))


def _resolve_slots(slots, width, levels, free_bytes, max_width):
    """-> the slots of a batch at most (a power of two).  ``free_bytes``: free device memory, or None if unknown"""
    need = lambda s: (levels + 2) * (16 << width) * s       # noqa: E731  (a source per level that still owes a run, the batch, a leaf)
    if slots is None:
        s = default_slots(width)
        while s > 1 and (width + s.bit_length() - 1 > max_width or (free_bytes is not None and need(s) > 0.8 * free_bytes)):
            s //= 2
        slots = s
    else:
        if isinstance(slots, bool) or int(slots) != slots or slots < 1 or (int(slots) & (int(slots) - 1)):
            raise ValueError("trajectory_slots must be a power of two >= 1, not %r" % (slots,))
        slots = int(slots)
        if width + slots.bit_length() - 1 > max_width:
            raise MemoryError("trajectory_slots=%d: a batch of %d slots of %d live qubits is a state of %d bytes (limit %d qubits)"
                              % (slots, slots, width, (16 << width) * slots, max_width))
    if free_bytes is not None and need(slots) > 0.8 * free_bytes:
        raise MemoryError("trajectory_slots=%d: %d engines of %d bytes each need %d bytes, 80 %% of the free device memory "
                          "is %d bytes" % (slots, levels + 2, (16 << width) * slots, need(slots), int(0.8 * free_bytes)))
    return slots


def run_trajectories(circuit, shots, seed, fusion=3, device=0, engine_factory=None, max_width=33, walk="depth", slots=None,
                     trace=None):
    """returns (values, counts, num_clbits, creg_sizes, metadata); values are the classical-register integers, a uint64
    array up to 64 classical bits and an object array of Python ints beyond.

    walk   "depth" (default): one engine per branch, the tree of outcomes depth first, one launch group and one host
           synchronisation per node.  "levels": the live branches of a level are the slots of one wider engine (slot b =
           the 2^w amplitudes from b << w): one ``exec`` per batch, one ``branch_mass`` for all its measurements, one
           vectorised binomial draw, one ``branch_split`` per run of at most ``slots`` children.
    slots  (levels walk) slots of a batch at most, a power of two; None: ``default_slots(w)``, halved while levels + 2
           engines of that size exceed 80 % of the free device memory.  An explicit value that cannot fit is a MemoryError.
    trace  (levels walk) a list: every measuring batch appends (level, [bits], [k], [mass0], [mass1], [k1]).

    The counts are a pure function of (circuit, shots, seed, fusion, walk, resolved slots).  The two walks, and two values
    of ``slots``, draw their random numbers in different orders: their counts agree statistically, not shot by shot."""
    if walk not in ("depth", "levels"):
        raise ValueError("unknown trajectory walk %r; the outcome tree is walked by 'depth' or by 'levels'" % (walk,))
    if walk == "depth" and slots is not None:
        raise ValueError("trajectory_slots belongs to the walk by 'levels'; the walk by 'depth' keeps one branch per engine")
    t0 = time.perf_counter()
    segs, width, final_measures, num_clbits, creg_sizes, n_src = compile_trajectory(circuit, fusion)
    if width > max_width:
        raise MemoryError("trajectory mode still needs %d live qubits (limit %d)" % (width, max_width))
    make = engine_factory or _lib.Engine
    rng = np.random.RandomState(seed % (2 ** 32))
    wide = num_clbits > 64
    fm_slots = [s for s, _ in final_measures]
    out_vals, out_cnts = [], []
    stats = {"nodes": 0, "copies": 0, "sweeps": 0, "engines": 0, "batches": 0, "max_batch_slots": 0, "in_use": 0,
             "max_in_use": 0, "t_leaves": 0.0}

    def leaf(eng, k, bits):
        """joint sample of what is left"""
        if fm_slots:
            smp = eng.sample(k, int(rng.randint(0, 2 ** 31 - 1)), fm_slots)
            uv, uc = _leaf_values(bits, smp, final_measures, wide)
            out_vals.extend(uv)
            out_cnts.extend(uc)
        else:
            out_vals.append(bits)
            out_cnts.append(k)

    t1 = time.perf_counter()
    if walk == "depth":
        _walk_depth(segs, width, make, device, rng, leaf, stats, int(shots))
        resolved = None
    else:
        free = _lib.device_memory(device)[0] if engine_factory is None else getattr(engine_factory, "free_bytes", None)
        resolved = _resolve_slots(slots, width, len(segs), free, max_width)
        _walk_levels(segs, width, make, device, rng, leaf, stats, resolved, int(shots), trace)
    t2 = time.perf_counter()
    if wide:
        vals = np.empty(len(out_vals), dtype=object)
        vals[:] = out_vals
    else:
        vals = np.asarray(out_vals, dtype=np.uint64)
    cnts = np.asarray(out_cnts, dtype=np.int64)
    meta = {"method": "trajectory", "live_qubits": width, "n_segments": len(segs), "n_source_ops": n_src,
            "branch_nodes": stats["nodes"], "state_copies": stats["copies"], "device_ops": stats["sweeps"],
            "engines": stats["engines"], "time_compile": t1 - t0, "time_evolve": t2 - t1, "trajectory_walk": walk,
            "trajectory_slots": resolved, "batches": stats["batches"], "max_batch_slots": stats["max_batch_slots"],
            "max_engines_in_use": stats["max_in_use"], "time_leaves": stats["t_leaves"]}
    return vals, cnts, num_clbits, creg_sizes, meta


def _walk_depth(segs, width, make, device, rng, leaf, stats, shots):
    pool = []
    created = []

    def get_engine():
        if pool:
            return pool.pop()
        e = make(width, devices=(device,))
        created.append(e)
        return e

    def node(level, eng, k, bits, came_by):
        sg = segs[level]
        stats["nodes"] += 1
        stats["sweeps"] += sg.n_ops
        rec, data = (sg.rec, sg.data) if came_by is None else sg.prog[came_by]
        if len(rec):
            eng.exec(rec, data)
        if sg.measure_slot is None:
            leaf(eng, k, bits)
            return
        # mass on outcome 1 and total mass in one read pass with a FIXED summation order (qsv_expect_diag: per-workgroup
        # partial sums, no atomics): the same seed walks the same tree on every run
        p1, tot = eng.expect_diag([sg.measure_slot], _ONE)
        k1 = int(rng.binomial(k, min(max(p1 / tot, 0.0), 1.0))) if tot > 0 else 0
        k0 = k - k1
        other = None
        if k0 > 0 and k1 > 0:
            other = get_engine()
            other.copy_from(eng)
            stats["copies"] += 1
        # the projection on the outcome (and the X that hands a released slot back) ride in front of the child's program
        for outcome, kk, e in ((0, k0, eng), (1, k1, other if other is not None else eng)):
            if kk:
                node(level + 1, e, kk, bits | (outcome << sg.measure_clbit), outcome)
        if other is not None:
            pool.append(other)

    try:
        node(0, get_engine(), shots, 0, None)
    finally:
        for e in created:
            e.close()
        stats["engines"] = len(created)


def _walk_levels(segs, width, make, device, rng, leaf, stats, slots, shots, trace):
    """The outcome tree level by level.  A batch is an engine of width + b qubits whose first B <= 2^b slots hold the live
    branches of one level, with their shots and register bits.  The last segment (nothing is measured after it) runs per
    leaf: ``branch_split`` always projects, so a branch is extracted from its PARENT batch into an engine of ``width``
    qubits, evolved through the last segment and sampled there."""
    pool = {}                                               # width -> idle engines
    alive = {}                                              # id -> (engine, amplitudes), idle ones included
    cap = (len(segs) + 2) * slots << width                  # amplitudes alive at once at most (the memory rule)
    last = len(segs) - 1

    def get_engine(w_eng):
        stats["in_use"] += 1
        stats["max_in_use"] = max(stats["max_in_use"], stats["in_use"])
        if pool.get(w_eng):
            return pool[w_eng].pop()
        # idle engines of other widths make room first: the engines in use are one source per level at most, the batch
        # and a leaf, each of at most ``slots`` slots
        while sum(a for _, a in alive.values()) + (1 << w_eng) > cap:
            wv = next((v for v in sorted(pool) if pool[v]), None)
            if wv is None:
                break
            e = pool[wv].pop()
            del alive[id(e)]
            e.close()
        e = make(w_eng, devices=(device,))
        alive[id(e)] = (e, 1 << w_eng)
        stats["engines"] += 1
        return e

    def put_engine(e):
        stats["in_use"] -= 1
        pool.setdefault(e.n_qubits, []).append(e)

    def leaves(src, sg, parents, outcomes, ks, bitsl):
        t_in = time.perf_counter()
        for p, o, k, bits in zip(parents, outcomes, ks, bitsl):
            e = get_engine(width)
            e.branch_split(src, width, [p], [o], sg.measure_slot, sg.release)
            stats["copies"] += 1
            stats["nodes"] += 1
            stats["sweeps"] += segs[last].n_ops
            if len(segs[last].rec):
                e.exec(segs[last].rec, segs[last].data)
            leaf(e, k, bits)
            put_engine(e)
        stats["t_leaves"] += time.perf_counter() - t_in

    def batch(eng, level, ks, bitsl):
        """``eng`` holds len(ks) branches that have not run segment ``level`` yet; owns ``eng`` (hands it back to the pool)"""
        sg = segs[level]
        B = len(ks)
        stats["batches"] += 1
        stats["max_batch_slots"] = max(stats["max_batch_slots"], B)
        stats["nodes"] += B
        stats["sweeps"] += sg.n_ops
        if len(sg.rec):
            eng.exec(sg.rec, sg.data)
        mass = np.asarray(eng.branch_mass(width, B, sg.measure_slot), dtype=np.float64).reshape(B, 2)
        tot = mass[:, 0] + mass[:, 1]
        if not np.all(tot > 0):
            b = int(np.flatnonzero(~(tot > 0))[0])
            raise RuntimeError("trajectory walk: the branch in slot %d of level %d holds %d shots and no mass "
                               "(register bits %s)" % (b, level, ks[b], bin(bitsl[b])))
        kv = np.asarray(ks, dtype=np.int64)
        k1 = rng.binomial(kv, np.clip(mass[:, 1] / tot, 0.0, 1.0))       # one vectorised call, in slot order
        k1 = np.asarray(k1, dtype=np.int64).reshape(B)
        if trace is not None:
            trace.append((level, list(bitsl), [int(k) for k in ks], mass[:, 0].tolist(), mass[:, 1].tolist(), k1.tolist()))
        parents, outcomes, cks, cbits = [], [], [], []
        for b in range(B):                                  # parents in slot order, outcome 0 before outcome 1
            for o, kk in ((0, int(kv[b] - k1[b])), (1, int(k1[b]))):
                if kk:
                    parents.append(b)
                    outcomes.append(o)
                    cks.append(kk)
                    cbits.append(bitsl[b] | (o << sg.measure_clbit))
        if level + 1 == last:                               # the children are leaves: one by one out of this batch
            leaves(eng, sg, parents, outcomes, cks, cbits)
            put_engine(eng)
            return
        runs = [(i, min(i + slots, len(cks))) for i in range(0, len(cks), slots)]
        for n, (i, j) in enumerate(runs):
            child = get_engine(width + (j - i - 1).bit_length())
            child.branch_split(eng, width, parents[i:j], outcomes[i:j], sg.measure_slot, sg.release)
            stats["copies"] += 1
            if n == len(runs) - 1:                          # a source is held only while a further run still needs it
                put_engine(eng)
            batch(child, level + 1, cks[i:j], cbits[i:j])

    try:
        root = get_engine(width)
        if last == 0:                                       # no mid-circuit measurement at all: the root is the leaf
            stats["nodes"] += 1
            stats["sweeps"] += segs[0].n_ops
            if len(segs[0].rec):
                root.exec(segs[0].rec, segs[0].data)
            leaf(root, shots, 0)
        else:
            batch(root, 0, [shots], [0])
    finally:
        for e, _ in alive.values():
            e.close()
