"""Cases and exact references of the shard-bit exchange and of the multi-rank sampling merge (test infrastructure; numpy
and ``math`` only besides the package's own host code).

Exchange.  ``qsv_swap_layout(pairs)`` swaps index BITS: the state after the call holds at global index g what stood at
the index with the bits of every pair exchanged, pair after pair in call order.  ``permute`` says exactly that and
nothing else.  A state that encodes its own index, ``amp[g] = g - 1j * g``, turns every comparison into
``np.array_equal`` and every failure into "index g holds what belonged to index s".

``block_model`` restates HOW libqsv gets there (``qsv_swap_layout`` / ``exchange_multi`` in qsv_layout.inc): local pairs
as sweeps, all shard-bit pairs of a call on distinct qubits as ONE step in which shard s trades, with every other member
of its group of 2^k shards, the block whose local bits J spell the partner's shard-bit values -- values deposited at the
J positions in PAIR order, each pair of shards splitting the block's index range in halves.  Its three switches are the
mistakes that code could make; test_exchange_cases.py shows that each differs from ``permute`` on every case it could
touch, so that an equality on the GPU means something.

Which form of ``k_swap_blocks`` a call runs (``single_swz`` / ``exchange_multi``): the index swizzle of the one-gate
kernels, bits 5 and 11 of the block index exchanged, when the engine swizzles at all (``swizzle`` 1 and L >= 26, or
``swizzle`` 2 and L >= 14), every swapped local bit is at least 6, and none is 5 or 11.  W = 15 on 2 shards and W = 16
on 4 both give L = 14, the smallest size at which ``swizzle`` 2 selects it.

Sampling.  RUNS lists the multi-rank ``run()`` calls whose merged counts tests/_gpu_rank_exact_worker.py rebuilds shot
by shot; the seeds are chosen here, on the CPU, so that no uniform of any rank lies near a prefix boundary
(``seed_margin``, ``closest_boundary``)."""
from __future__ import annotations

import collections
import functools
import itertools
import math

import numpy as np

SWAP_U = np.array([[0.5, 1j], [2.0, -1.0]])        # dyadic entries: every product and sum below is exact in float64


def log2i(P):
    return int(P).bit_length() - 1


def encode_state(W):
    """amp[g] = g - 1j * g"""
    g = np.arange(1 << W, dtype=np.float64)
    return g - 1j * g


def swap_bits(idx, a, b):
    d = ((idx >> a) ^ (idx >> b)) & 1
    return idx ^ (d << a) ^ (d << b)


def permute(W, pairs):
    """src with state_after[g] == state_before[src[g]] for the swaps ``pairs`` = [(a, b), ...] applied in order"""
    idx = np.arange(1 << W, dtype=np.int64)
    src = idx.copy()
    for a, b in pairs:
        if a != b:
            src = src[swap_bits(idx, a, b)]
    return src


# ---------------------------------------------------------------------------------------------------------------------
# the rule as written in qsv_swap_layout / exchange_multi / single_swz
# ---------------------------------------------------------------------------------------------------------------------
def exchange_calls(W, P, pairs):
    """the exchange steps of one call, in order, as (G, J) lists (shard bits, local bits, pair order)"""
    L = W - log2i(P)
    live = [(a, b) for a, b in pairs if a != b]
    seen, disjoint = set(), True
    for a, b in live:
        if a in seen or b in seen:
            disjoint = False
        seen |= {a, b}
    calls, G, J = [], [], []
    for a, b in live:
        lo, hi = min(a, b), max(a, b)
        if hi < L:
            continue
        if disjoint:
            G.append(hi)
            J.append(lo)
        else:
            calls.append(([hi], [lo]))
    if G:
        calls.append((G, J))
    return calls


def call_swizzled(L, J, swizzle):
    on = bool(swizzle) and (L >= 26 or (swizzle > 1 and L >= 14))
    return on and min(J) >= 6 and not any(j in (5, 11) for j in J)


Case = collections.namedtuple("Case", "name W P a b exchanges swizzled")


def _case(name, W, P, pairs):
    calls = exchange_calls(W, P, pairs)
    L = W - log2i(P)
    return Case(name, W, P, [p[0] for p in pairs], [p[1] for p in pairs], len(calls),
                any(call_swizzled(L, J, 2) for _, J in calls))


K1_J = (0, 5, 6, 11, 13)
K2_J = ((0, 3), (5, 11), (6, 12), (13, 2), (12, 13), (11, 7))
FORMS = ((15, 2), (16, 4))              # (W, P): L = 14


@functools.lru_cache(maxsize=None)
def form_cases():
    """the table at L = 14"""
    out = []
    for W, P in FORMS:
        L = W - log2i(P)
        shard_bits = list(range(L, W))
        n = 0
        for j in K1_J:
            for G in shard_bits:
                n += 1
                out.append(_case("P%d_k1_J%d_G%d" % (P, j, G), W, P, [(G, j) if n % 2 else (j, G)]))
        if P == 4:
            for j0, j1 in K2_J:
                for order, (G0, G1) in enumerate(((L, L + 1), (L + 1, L))):
                    # the shard bit on either side of a pair, the sides changing with the assignment
                    pairs = [(G0, j0), (j1, G1)] if order == 0 else [(j0, G0), (G1, j1)]
                    out.append(_case("P4_k2_J%d_%d_G%d_%d" % (j0, j1, G0, G1), W, P, pairs))
        top = W - 1
        out.append(_case("P%d_local_pair_mixed_in" % P, W, P, [(2, 9), (top, 3), (12, 7)] if P == 2 else [(2, 9), (top, 3), (12, 7), (8, L)]))
        out.append(_case("P%d_shared_qubit" % P, W, P, [(top, 4), (4, 9), (5, L)]))
        out.append(_case("P%d_equal_pair" % P, W, P, [(3, 3), (top, 6), (top, top), (7, 7)]))
        out.append(_case("P%d_empty" % P, W, P, []))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def small_cases():
    """k = L (one block per shard: the lower shard of a pair moves nothing, the higher one the whole block) and L = 3"""
    out = [_case("W2_P2_k1", 2, 2, [(1, 0)]),
           _case("W3_P4_k1_G1", 3, 4, [(0, 1)]),
           _case("W3_P4_k1_G2", 3, 4, [(2, 0)]),
           _case("W4_P4_k2", 4, 4, [(2, 0), (1, 3)]),
           _case("W4_P4_k2_crossed", 4, 4, [(0, 3), (2, 1)]),
           _case("W4_P4_k2_descending", 4, 4, [(2, 1), (3, 0)])]
    out += [_case("W4_P2_L3_J%d" % j, 4, 2, [(3, j) if j != 1 else (j, 3)]) for j in range(3)]
    out += [_case("W5_P4_L3_G3_J1", 5, 4, [(3, 1)]), _case("W5_P4_L3_G4_J2", 5, 4, [(2, 4)]),
            _case("W5_P4_L3_k2", 5, 4, [(4, 0), (2, 3)])]
    return tuple(out)


def all_cases():
    return form_cases() + small_cases()


@functools.lru_cache(maxsize=None)
def expected_state(name):
    c = {c.name: c for c in all_cases()}[name]
    out = encode_state(c.W)[permute(c.W, list(zip(c.a, c.b)))]
    out.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# sequences: every step is ("swap", a, b) or ("u", target, matrix); compared after every step
# ---------------------------------------------------------------------------------------------------------------------
def _alternating(L):
    js = [0, 5, 6, 11, 13, 3, 7, 12, 1, 9, 10, 2, 8, 4, 6, 13]
    steps, n = [], 0
    for i in range(12):
        if i % 3 == 0:
            steps.append(("swap", [L], [js[n]]))
            n += 1
        elif i % 3 == 1:
            steps.append(("swap", [js[n]], [L + 1]))
            n += 1
        else:
            steps.append(("swap", [L + 1, js[n]], [js[n + 1], L]))
            n += 2
    return steps


SEQUENCES = {
    # name: (W, P, steps)
    "P4_alternating_groups": (16, 4, _alternating(14)),
    "P2_gate_behind_exchange": (15, 2, [("swap", [14], [6]), ("u", 6, SWAP_U), ("swap", [6], [14])]),
    "P4_gate_behind_exchange": (16, 4, [("swap", [14, 12], [6, 15]), ("u", 6, SWAP_U), ("u", 12, SWAP_U),
                                        ("swap", [14, 12], [6, 15]), ("swap", [15], [0]), ("u", 0, SWAP_U), ("swap", [0], [15])]),
}


def sequence_exchanges(name):
    W, P, steps = SEQUENCES[name]
    return [len(exchange_calls(W, P, list(zip(st[1], st[2])))) if st[0] == "swap" else 0 for st in steps]


@functools.lru_cache(maxsize=None)
def sequence_states(name):
    """the state after every step, from encode_state(W)"""
    W, P, steps = SEQUENCES[name]
    v = encode_state(W)
    out = []
    for st in steps:
        if st[0] == "swap":
            v = v[permute(W, list(zip(st[1], st[2])))]
        else:
            t, m = st[1], np.asarray(st[2])
            x = v.reshape(-1, 2, 1 << t)
            v = np.stack([m[0, 0] * x[:, 0] + m[0, 1] * x[:, 1], m[1, 0] * x[:, 0] + m[1, 1] * x[:, 1]], axis=1).reshape(-1)
        v.setflags(write=False)
        out.append(v)
    return tuple(out)


def first_mismatch(got, want, base=0):
    """text for an assertion: the first global index that differs and whose amplitude it holds instead"""
    bad = np.flatnonzero(got != want)
    if bad.size == 0:
        return ""
    i = int(bad[0])
    return "%d of %d differ; index %d holds %r, expected %r" % (bad.size, got.size, base + i, complex(got[i]), complex(want[i]))


# ---------------------------------------------------------------------------------------------------------------------
# the mechanism, with its possible mistakes
# ---------------------------------------------------------------------------------------------------------------------
def ins_bits(p, positions):
    for pos in sorted(positions):
        p = ((p >> pos) << (pos + 1)) | (p & ((1 << pos) - 1))
    return p


def deposit_bits(v, positions):
    return sum(((v >> i) & 1) << pos for i, pos in enumerate(positions))


def _group_value(shard, gb):
    return sum(((shard >> b) & 1) << i for i, b in enumerate(gb))


def _with_group_value(shard, gb, v):
    for i, b in enumerate(gb):
        shard = (shard & ~(1 << b)) | (((v >> i) & 1) << b)
    return shard


def block_model(W, P, pairs, sorted_j=False, as_disjoint=False, low_half_only=False):
    """``permute`` by the engine's steps.  sorted_j: block values deposited at the J positions in ascending order instead
    of pair order.  as_disjoint: a call whose pairs share a qubit run like one whose pairs do not (local pairs at once,
    shard-bit pairs behind them).  low_half_only: both shards of a pair take the lower shard's half of the block's index
    range, so the upper half never moves."""
    L = W - log2i(P)
    n = 1 << L
    src = np.arange(1 << W, dtype=np.int64).reshape(P, n).copy()
    idx = np.arange(n, dtype=np.int64)

    def local(lo, hi):
        for s in range(P):
            src[s] = src[s][swap_bits(idx, lo, hi)]

    def exchange(G, J):
        k = len(G)
        gb = [g - L for g in G]
        nblock = n >> k
        half = nblock >> 1
        at = sorted(J) if sorted_j else J
        rest = ins_bits(np.arange(nblock, dtype=np.int64), J)
        for s in range(P):
            me = _group_value(s, gb)
            for v in range(1 << k):
                if v == me:
                    continue
                peer = _with_group_value(s, gb, v)
                low = me < v
                if low_half_only and not low:
                    continue
                p0, cnt = (0, half) if low else (half, nblock - half)
                i = rest[p0:p0 + cnt]
                fa, fb = deposit_bits(v, at), deposit_bits(me, at)
                x = src[s][i | fa].copy()
                src[s][i | fa] = src[peer][i | fb]
                src[peer][i | fb] = x

    live = [(min(a, b), max(a, b)) for a, b in pairs if a != b]
    flat = [q for p in live for q in p]
    disjoint = as_disjoint or len(set(flat)) == len(flat)
    G, J = [], []
    for lo, hi in live:
        if hi < L:
            local(lo, hi)
        elif disjoint:
            G.append(hi)
            J.append(lo)
        else:
            exchange([hi], [lo])
    if G and len(set(G)) == len(G):
        exchange(G, J)
    else:                                  # (as_disjoint on a call that repeats a shard bit: one after the other, still late)
        for g, j in zip(G, J):
            exchange([g], [j])
    return src.reshape(-1)


# ---------------------------------------------------------------------------------------------------------------------
# multi-rank sampling: circuits with a closed form, the runs, their seeds
# ---------------------------------------------------------------------------------------------------------------------
SHOTS = 6000
WIDTH = 16
SEED_MUL = 1315423911                   # rank r of a run draws with (seed * SEED_MUL + r) mod 2^63 (backend._run_one)


def rank_seed(seed, rank):
    return (seed * SEED_MUL + rank) % (2 ** 63)


def shot_split(seed, shots, masses):
    """the documented split of a run's shots over the ranks: one multinomial draw, the same on every rank"""
    masses = np.asarray(masses, dtype=np.float64)
    return np.random.RandomState(seed % (2 ** 32)).multinomial(shots, masses / masses.sum())


def _sparse_angles():
    rs = np.random.RandomState(5)
    return rs.uniform(0.3, 2.8, size=13), rs.uniform(0.1, 3.0, size=12)


def sparse_circuit():
    """16 qubits: 0..12 rotated and phase-coupled, 13 and 14 in uniform superposition and NOT measured, 15 never touched;
    the 14 measured qubits land on scrambled classical bits, two classical bits stay unwritten"""
    from qcmrf_amd.circuit import QuantumCircuit
    ry, cp = _sparse_angles()
    qc = QuantumCircuit(WIDTH, WIDTH)
    qc.h(13)
    qc.h(14)
    for q in range(13):
        qc.ry(float(ry[q]), q)
    for q in range(12):
        qc.cp(float(cp[q]), q, q + 1)
    for q in list(range(13)) + [15]:
        qc.measure(q, (5 * q + 3) % WIDTH)
    return qc


def sparse_amplitudes():
    ry, cp = _sparse_angles()
    idx = np.arange(1 << WIDTH, dtype=np.int64)
    amp = np.full(idx.size, 0.5, dtype=np.complex128)          # qubits 13, 14
    for q in range(13):
        bit = (idx >> q) & 1
        amp *= np.where(bit == 1, math.sin(ry[q] / 2), math.cos(ry[q] / 2))
    for q in range(12):
        amp *= np.where(((idx >> q) & (idx >> (q + 1)) & 1) == 1, np.exp(1j * cp[q]), 1.0)
    amp[(idx >> 15) & 1 == 1] = 0
    return amp


@functools.lru_cache(maxsize=None)
def circuit_of(name):
    """(circuit, closed-form amplitudes by LOGICAL index, [(qubit, classical bit), ...] read off the circuit)"""
    if name == "chain8":
        from oracle import closed_form as cf
        from qcmrf_amd import QCMRF, workloads
        C = workloads.chain(8)
        th = workloads.theta_halfnorm(workloads.dimension(C))
        qc, amp = QCMRF(C, th), cf.amplitudes(C, th)
    else:
        qc, amp = sparse_circuit(), sparse_amplitudes()
    measured = [(qc.find_bit(ci.qubits[0]).index, qc.find_bit(ci.clbits[0]).index) for ci in qc.data if ci.operation.name == "measure"]
    amp.setflags(write=False)
    return qc, amp, measured


Run = collections.namedtuple("Run", "circuit layout fusion fold_fresh gather engine_options seeds")

# seeds: world size -> seed_simulator, chosen by test_exchange_cases.py's rule (no uniform of any rank within
# seed_margin of a prefix boundary)
RUNS = {
    "chain8_reference_fused": Run("chain8", "reference", 2, False, "root", {}, {2: 11, 4: 12}),
    "chain8_reference_gate_by_gate": Run("chain8", "reference", 0, False, "root", {}, {2: 13, 4: 14}),
    "chain8_auto_folded_all": Run("chain8", "auto", 3, True, "all", {}, {2: 15, 4: 16}),
    "chain8_auto_sweeps": Run("chain8", "auto", 2, False, "root", {}, {2: 17, 4: 18}),
    "chain8_reference_index_order_all": Run("chain8", "reference", 2, False, "all", {"fused_sums": 0}, {2: 19, 4: 20}),
    "sparse_reference_empty_ranks": Run("sparse", "reference", 2, False, "root", {}, {2: 21, 4: 22}),
    "sparse_auto_index_order": Run("sparse", "auto", 3, True, "root", {"fused_sums": 0}, {2: 23, 4: 24}),
}


def run_options(run):
    return dict(layout=run.layout, fusion=run.fusion, fold_fresh=run.fold_fresh, gather_counts=run.gather,
                engine_options=dict(run.engine_options) or None)


@functools.lru_cache(maxsize=None)
def plan_of(name, world):
    """the plan of a run on ``world`` ranks (host code only)"""
    from qcmrf_amd.backend import QsvBackend
    run = RUNS[name]
    _, pl = QsvBackend().compile(circuit_of(run.circuit)[0], world, layout=run.layout, fusion=run.fusion,
                                 fold_fresh=run.fold_fresh, engine_options=dict(run.engine_options) or None)
    return pl


def expects_index_order(run, op_kinds):
    """Whether a rank's draw takes the block-sum walk in ascending index (a QSV_K_PROB launch) and not the tile walk.
    The tile sums are those of the program's last pass: ``fused_sums`` 0 forms none, an exchange drops them, and a last
    pass of ONE op runs as that op's own kernel, which leaves none (``flush_group``, single_shortcut) -- the reference
    layout on two ranks ends ``swap, mux``."""
    if run.engine_options.get("fused_sums") == 0:
        return True
    kinds = list(op_kinds)
    tail = kinds[len(kinds) - kinds[::-1].index("swap"):] if "swap" in kinds else kinds
    return len(tail) <= 1


def logical_of_physical(layout, start, count):
    """logical index of the physical indices [start, start + count): layout[logical qubit] = physical bit"""
    p = np.arange(start, start + count, dtype=np.int64)
    l = np.zeros_like(p)
    for q, pos in enumerate(layout):
        l |= ((p >> pos) & 1) << q
    return l


def clbit_values(words, layout, measured):
    """raw sampled words (global physical indices) -> classical register values, bit c <- the qubit measured into c"""
    w = np.asarray(words, dtype=np.uint64)
    out = np.zeros(w.shape, dtype=np.uint64)
    for q, c in measured:
        out |= ((w >> np.uint64(layout[q])) & np.uint64(1)) << np.uint64(c)
    return out


def counts_dict(values, num_clbits):
    uv, uc = np.unique(np.asarray(values, dtype=np.uint64), return_counts=True)
    return {format(int(v), "0%db" % num_clbits): int(c) for v, c in zip(uv, uc)}


def probs(v):
    v = np.asarray(v, dtype=np.complex128)
    return v.real * v.real + v.imag * v.imag


def seed_margin(p_shard, total):
    """How far from every prefix boundary a uniform has to stay, on the closed-form probabilities, for the word it draws
    on the device to be certain.  Three terms: the sampler's own tolerance TOL_REL * total; the uniforms scale with the
    engine's total, within 1e-12 of this one; and a prefix sum of the device's |amp|^2 differs from this one by at most
    sum 2 |a| 1e-12 <= 2e-12 sqrt(populated * total) when every amplitude is within the suite's 1e-12 of the closed form."""
    from _sampler_reference import TOL_REL
    populated = int(np.count_nonzero(p_shard))
    return TOL_REL * total + 1e-12 * total + 2e-12 * math.sqrt(populated * total)


def closest_boundary(p_shard, seed, shots):
    """(distance of the nearest uniform to a prefix boundary, margin) for one rank's draw of ``shots`` words"""
    from _sampler_reference import exact_index_order, sorted_uniforms
    total = math.fsum(p_shard.tolist())
    r = sorted_uniforms(seed, shots, total)
    _, dist = exact_index_order(p_shard, r)
    return float(dist.min()), seed_margin(p_shard, total)


def possible_splits(seed, shots, masses, eps=1e-12):
    """every split of the shots that per-rank masses within ``eps`` of ``masses`` can give"""
    masses = np.asarray(masses, dtype=np.float64)
    out = set()
    for signs in itertools.product((-1.0, 0.0, 1.0), repeat=len(masses)):
        m = np.maximum(masses + eps * np.asarray(signs), 0.0) * (masses > 0)
        out.add(tuple(int(x) for x in shot_split(seed, shots, m)))
    return sorted(out)
