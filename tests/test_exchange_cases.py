"""CPU: the case table and references of the exchange and multi-rank sampling tests (_exchange_cases.py) are what they
claim to be -- ``permute`` against the numpy engine, the expected exchange counts and swizzled forms against the rule,
every mistake the block mechanism could make rejected, and no uniform of the chosen seeds near a prefix boundary."""
import math

import numpy as np
import pytest

import _exchange_cases as xc
from oracle.sharded_numpy import NumpyEngine


def _loaded(W, P):
    ref = NumpyEngine(W, P)
    st = xc.encode_state(W)
    L = W - xc.log2i(P)
    for s in range(P):
        ref.sh[s][:] = st[s << L:(s + 1) << L]
    return ref


@pytest.mark.parametrize("case", xc.all_cases(), ids=lambda c: c.name)
def test_permute_is_the_numpy_engines_swap_layout(case):
    ref = _loaded(case.W, case.P)
    ref.swap_layout(case.a, case.b)
    want = xc.expected_state(case.name)
    assert np.array_equal(ref.amplitudes(), want), xc.first_mismatch(ref.amplitudes(), want)
    assert ref.stats()["exchanges"] == case.exchanges
    pairs = list(zip(case.a, case.b))
    assert np.array_equal(xc.block_model(case.W, case.P, pairs), xc.permute(case.W, pairs))     # the mechanism, unmutated
    assert sorted(want.real.astype(np.int64).tolist()) == list(range(1 << case.W))              # a permutation


@pytest.mark.parametrize("name", sorted(xc.SEQUENCES))
def test_sequences_against_the_numpy_engine(name):
    W, P, steps = xc.SEQUENCES[name]
    ref = _loaded(W, P)
    want = xc.sequence_states(name)
    for k, st in enumerate(steps):
        if st[0] == "swap":
            ref.swap_layout(st[1], st[2])
        else:
            ref.apply_1q(st[1], st[2])
        assert np.array_equal(ref.amplitudes(), want[k]), (name, k, xc.first_mismatch(ref.amplitudes(), want[k]))
    assert ref.stats()["exchanges"] == sum(xc.sequence_exchanges(name))
    if name.endswith("gate_behind_exchange"):
        assert not np.array_equal(want[-1], xc.encode_state(W))           # the gates did something the inverse exchange kept
        L = W - xc.log2i(P)
        for k, st in enumerate(steps):
            if st[0] == "u":                                              # ... on a bit the step before swapped in
                prev = steps[k - 1] if steps[k - 1][0] == "swap" else steps[k - 2]
                assert st[1] in [min(a, b) for a, b in zip(prev[1], prev[2]) if max(a, b) >= L]


def test_alternating_sequence_changes_its_peer_groups():
    W, P, steps = xc.SEQUENCES["P4_alternating_groups"]
    L = W - xc.log2i(P)
    groups = [tuple(sorted(max(a, b) for a, b in zip(st[1], st[2]))) for st in steps]
    assert len(steps) == 12 and groups == [(L,), (L + 1,), (L, L + 1)] * 4
    assert xc.sequence_exchanges("P4_alternating_groups") == [1] * 12
    js = [tuple(min(a, b) for a, b in zip(st[1], st[2])) for st in steps]
    assert len(set(js)) == 12


def test_table_holds_what_the_issue_lists():
    cases = xc.form_cases()
    by = {c.name: c for c in cases}
    assert len(by) == len(cases)
    for W, P in xc.FORMS:
        assert W - xc.log2i(P) == 14
        for j in xc.K1_J:
            for G in range(14, W):
                c = by["P%d_k1_J%d_G%d" % (P, j, G)]
                assert sorted(zip(c.a, c.b)) in ([(G, j)], [(j, G)]) and c.exchanges == 1
                assert c.swizzled == (j in (6, 13)), c.name
        assert by["P%d_shared_qubit" % P].exchanges == 2
        assert by["P%d_equal_pair" % P].exchanges == 1 and by["P%d_empty" % P].exchanges == 0
        assert by["P%d_local_pair_mixed_in" % P].exchanges == 1
    sides = set()
    for j0, j1 in xc.K2_J:
        seen = set()
        for G0, G1 in ((14, 15), (15, 14)):
            c = by["P4_k2_J%d_%d_G%d_%d" % (j0, j1, G0, G1)]
            pairs = [(max(a, b), min(a, b)) for a, b in zip(c.a, c.b)]
            assert pairs == [(G0, j0), (G1, j1)] and c.exchanges == 1            # J in the order given, G in both orders
            assert c.swizzled == ((j0, j1) in ((6, 12), (12, 13))), c.name
            seen.add(tuple(pairs))
            sides |= {a > b for a, b in zip(c.a, c.b)}
        assert len(seen) == 2
    assert sides == {True, False}                                                  # the shard bit on either side of a pair
    assert {c.swizzled for c in cases} == {True, False}
    # the two forms are told apart by the rule alone: no swizzle, or a shard below 2^14 amplitudes, selects neither
    assert not xc.call_swizzled(14, [6], 0) and not xc.call_swizzled(14, [6], 1) and not xc.call_swizzled(13, [6], 2)
    assert xc.call_swizzled(26, [6], 1) and not xc.call_swizzled(26, [6, 11], 1) and not xc.call_swizzled(26, [4, 12], 2)


def test_small_cases_have_one_block_or_three_local_bits():
    one_block = [c for c in xc.small_cases() if "_L3_" not in c.name]
    assert sorted({(c.W, c.P) for c in one_block}) == [(2, 2), (3, 4), (4, 4)]
    for c in one_block:
        L = c.W - xc.log2i(c.P)
        (G, J), = xc.exchange_calls(c.W, c.P, list(zip(c.a, c.b)))
        assert len(G) == L and (1 << L) >> len(G) == 1                            # nblock = 1: half = 0
    for c in xc.small_cases():
        if "_L3_" in c.name:
            assert c.W - xc.log2i(c.P) == 3 and c.exchanges == 1


def _affected(case, mutation):
    pairs = list(zip(case.a, case.b))
    calls = xc.exchange_calls(case.W, case.P, pairs)
    if mutation == "sorted_j":
        return any(J != sorted(J) for _, J in calls)
    if mutation == "as_disjoint":
        live = [q for a, b in pairs if a != b for q in (a, b)]
        return len(set(live)) != len(live)
    return len(calls) > 0


@pytest.mark.parametrize("mutation", ["sorted_j", "as_disjoint", "low_half_only"])
def test_each_mistake_of_the_mechanism_changes_every_case_it_touches(mutation):
    hit = 0
    for c in xc.all_cases():
        pairs = list(zip(c.a, c.b))
        got = xc.block_model(c.W, c.P, pairs, **{mutation: True})
        same = np.array_equal(got, xc.permute(c.W, pairs))
        assert same != _affected(c, mutation), (mutation, c.name)
        hit += not same
    assert hit >= {"sorted_j": 4, "as_disjoint": 2, "low_half_only": 40}[mutation]
    for name, (W, P, steps) in xc.SEQUENCES.items():                              # ... and every exchange of the sequences
        for st in steps:
            if st[0] == "swap" and mutation == "low_half_only":
                pairs = list(zip(st[1], st[2]))
                assert not np.array_equal(xc.block_model(W, P, pairs, low_half_only=True), xc.permute(W, pairs)), name


# ---------------------------------------------------------------------------------------------------------------------
# multi-rank sampling
# ---------------------------------------------------------------------------------------------------------------------
def test_sparse_circuit_closed_form():
    from qcmrf_amd.backend import QsvBackend
    qc, amp, measured = xc.circuit_of("sparse")
    be = QsvBackend()
    be._engine_factory = lambda n, devices=(0,), rank=None, world_size=None: NumpyEngine(n, len(devices))
    be.run(qc, shots=0, seed_simulator=1)
    assert np.abs(be.statevector() - amp).max() < 1e-13
    assert abs(math.fsum(xc.probs(amp).tolist()) - 1.0) < 1e-13
    qs, cs = [q for q, _ in measured], [c for _, c in measured]
    assert sorted(qs) == list(range(13)) + [15] and len(set(cs)) == 14 and cs != qs


def _physical_probs(name, world):
    """(p by physical index, plan) of a run on ``world`` ranks, from the closed form and the plan alone"""
    _, amp, _ = xc.circuit_of(xc.RUNS[name].circuit)
    pl = xc.plan_of(name, world)
    return xc.probs(amp)[xc.logical_of_physical(pl.layout, 0, amp.size)], pl


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("name", sorted(xc.RUNS))
def test_no_uniform_of_the_chosen_seeds_is_ambiguous(name, world):
    """for every split of the shots that per-rank masses within 1e-12 of the closed form can give, every uniform of every
    rank's draw stays further from a prefix boundary of that rank's shard than ``seed_margin``"""
    run = xc.RUNS[name]
    p, pl = _physical_probs(name, world)
    L = xc.WIDTH - xc.log2i(world)
    shards = [p[r << L:(r + 1) << L] for r in range(world)]
    masses = [math.fsum(s.tolist()) for s in shards]
    seed = run.seeds[world]
    splits = xc.possible_splits(seed, xc.SHOTS, masses)
    assert splits and all(sum(s) == xc.SHOTS for s in splits)
    for split in splits:
        for r in range(world):
            assert (split[r] == 0) == (masses[r] == 0.0)
            if split[r]:
                dist, margin = xc.closest_boundary(shards[r], xc.rank_seed(seed, r), split[r])
                assert dist > margin, (name, world, r, split, dist, margin)


def test_runs_cover_what_they_are_there_for():
    empty, dup, exch, free, paths = set(), set(), set(), set(), set()
    for name, run in xc.RUNS.items():
        _, _, measured = xc.circuit_of(run.circuit)
        for world in (2, 4):
            p, pl = _physical_probs(name, world)
            L = xc.WIDTH - xc.log2i(world)
            masses = [float(p[r << L:(r + 1) << L].sum()) for r in range(world)]
            if min(masses) == 0.0:
                empty.add(world)
            shard_q = [q for q in range(xc.WIDTH) if pl.layout[q] >= L]
            if any(q not in [m[0] for m in measured] for q in shard_q) and sum(m > 0 for m in masses) > 1:
                dup.add(world)                           # populated ranks that differ in an unmeasured qubit: equal outcomes to merge
            (exch if pl.n_exchanges else free).add(world)
            paths.add((xc.expects_index_order(run, [o.kind for o in pl.ops]), bool(run.engine_options), bool(pl.n_exchanges)))
    assert empty == {2, 4} and dup == {2, 4} and exch == {2, 4} and free == {2, 4}
    assert {r.gather for r in xc.RUNS.values()} == {"root", "all"}
    # the block-sum walk by option and behind an exchange that dropped the tile sums; the tile walk with and without an exchange
    assert paths >= {(True, True, False), (True, False, True), (False, False, True), (False, False, False)}
    assert {(r.layout, r.fusion) for r in xc.RUNS.values()} >= {("reference", 2), ("reference", 0)}
    assert {(r.layout, r.fold_fresh) for r in xc.RUNS.values()} >= {("auto", True), ("auto", False)}


def test_counts_reference_maps_bits_in_numpy():
    """clbit_values / counts_dict against the backend's own formatter on a scrambled map"""
    from qcmrf_amd.backend import _format_keys
    rs = np.random.RandomState(3)
    words = rs.randint(0, 1 << 16, size=500).astype(np.uint64)
    layout = [int(x) for x in rs.permutation(16)]
    measured = [(q, (5 * q + 3) % 16) for q in range(0, 16, 2)]
    vals = xc.clbit_values(words, layout, measured)
    for w, v in zip(words.tolist()[:50], vals.tolist()[:50]):
        assert v == sum(((w >> layout[q]) & 1) << c for q, c in measured)
    uv, uc = np.unique(vals, return_counts=True)
    assert xc.counts_dict(vals, 16) == _format_keys(uv, uc, 16, [("c", 16)])
