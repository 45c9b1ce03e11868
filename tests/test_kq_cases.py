"""The case table of the matrix-core dense-gate tests (tests/_kq_cases.py) against its own model of the walks, on the
host: every batch of every row is computed exactly once and nothing is fetched from past the end, the rows reach every
walk shape the kernels have, and the model notices three planted mistakes.  Conditions, not measurements: a row that
stops reaching its shape (another grid rule in launch_kq_mfma, say) has to be replaced, not the condition dropped."""
import pytest

import _kq_cases as kc
from _kq_cases import ROWS


def lds_rows(pd):
    return [r for r in ROWS if r.variant == 5 + pd]


@pytest.mark.parametrize("n_cu", kc.N_CU)
def test_every_batch_once_and_every_fetch_real(n_cu):
    for row in ROWS:
        assert kc.defects(row, n_cu) == [], row


def test_rows_are_distinct_and_inside_the_sizes_the_suite_holds():
    assert len(set(ROWS)) == len(ROWS)
    for r in ROWS:
        assert kc.km_of(r.k) + 4 <= r.L <= kc.L_MAX and r.kq_grid in (0, 1, 3), r
        assert (r.nontemporal, r.swizzle) in kc.ACCESS
    for name, row in kc.REGRESSIONS.items():
        assert row in ROWS, name


@pytest.mark.parametrize("n_cu", kc.N_CU)
def test_a_cap_is_in_the_table_only_where_it_changes_the_grid(n_cu):
    for r in ROWS:
        if r.kq_grid:
            free = kc.launch(r.L, r.k, r.variant, 0, n_cu).grid
            assert kc.launch(r.L, r.k, r.variant, r.kq_grid, n_cu).grid == r.kq_grid < free, r


@pytest.mark.parametrize("n_cu", kc.N_CU)
@pytest.mark.parametrize("pd", [1, 2, 3])
def test_lds_walks_reach_every_shape(pd, n_cu):
    """k_kq_lds with PD loads in flight (kq_variant 5 + PD).  PD = 1 has no guarded tail and no wave with n_my < PD (a wave
    that stays has at least one batch): those two conditions are for PD = 2, 3"""
    residues, short, long_loop, uneven, returning, tails = set(), False, False, False, False, set()
    for row in lds_rows(pd):
        la, waves = kc.waves_of(row, n_cu)
        assert la.kernel == "lds" and la.pd == pd
        stay = [w for w in waves if not w.returned]
        for w in stay:
            residues.add(w.n_my % pd)
            tails.add(w.tail)
            assert w.peeled == (w.n_my >= pd) and w.tail == (w.n_my % pd if pd > 1 else 0)
            short |= not w.peeled
            long_loop |= w.peeled and w.rounds >= 2
        uneven |= len({w.n_my for w in stay}) >= 2
        returning |= len(stay) < len(waves)
    assert residues == set(range(pd))
    assert tails == set(range(pd))                   # PD = 3: the tail of one and the tail of two
    assert short == (pd > 1)
    assert long_loop and uneven and returning


@pytest.mark.parametrize("n_cu", kc.N_CU)
@pytest.mark.parametrize("chunked", [0, 1])
@pytest.mark.parametrize("kernel,variants", [("mfma", (0,)), ("mfma3", (1, 2, 3, 4))])
def test_mfma_walks_reach_every_shape(kernel, variants, chunked, n_cu):
    """k_kq_mfma and k_kq_mfma3, grid-stride and contiguous (kq_chunked); every variant of k_kq_mfma3 by itself, since PF
    and ALDS are template parameters"""
    for variant in variants:
        one, many, empty, short_last, skipped, taken = False, False, False, False, False, False
        for row in ROWS:
            if row.variant != variant or row.chunked != chunked:
                continue
            la, waves = kc.waves_of(row, n_cu)
            assert la.kernel == kernel and la.prefetch == (variant in (2, 3))
            for w in waves:
                one |= len(w.done) == 1
                many |= len(w.done) >= 32
                if kernel == "mfma3" and w.done:
                    assert w.more == [True] * (len(w.done) - 1) + [False]
                    skipped |= w.more == [False]     # no second batch: nothing requested on entry
                    taken |= len(w.more) > 1
                if chunked:
                    bt0, bt1, per = w.chunk
                    empty |= bt0 >= la.n
                    short_last |= 0 < bt1 - bt0 < per
        assert one and many, variant
        if kernel == "mfma3":
            assert skipped and taken, variant
        if chunked:
            assert empty and short_last, variant


@pytest.mark.parametrize("n_cu", kc.N_CU)
def test_wide_walk_reaches_one_step_many_steps_and_both_fallbacks(n_cu):
    one, many, fallback = False, False, set()
    for row in ROWS:
        if row.variant != 5:
            continue
        la, waves = kc.waves_of(row, n_cu)
        if kc.nbatch_of(row.L, row.k) % 2:
            assert la.kernel == "mfma3" and la.fallback and la.prefetch      # variant 3 in its place
            fallback.add((kc.km_of(row.k), row.L, row.chunked))
        else:
            assert la.kernel == "mfma3w" and la.n == kc.nbatch_of(row.L, row.k) // 2
            one |= la.n == 1
            many |= any(len(w.done) >= 32 for w in waves)
    assert one and many
    assert {(4, 8, 0), (4, 8, 1), (5, 9, 0), (5, 9, 1)} <= fallback


def test_blocks_per_cu_row_of_the_gpu_test_is_modelled():
    """kq_blocks_per_cu = 1 at L = 16, K = 5 (the one GPU case that sets the option): the grids it gives"""
    for variant in (3, 8):
        for n_cu in kc.N_CU:
            la = kc.launch(16, 5, variant, 0, n_cu, blocks_per_cu=1)
            assert la.grid == min(n_cu, 4 if variant == 3 else 2)


@pytest.mark.parametrize("n_cu", kc.N_CU)
@pytest.mark.parametrize("mistake", kc.MISTAKES)
def test_the_table_notices_a_planted_mistake(mistake, n_cu):
    """the PD = 3 tail handling only its first slot, a fetch index that is not clamped to the wave's last batch, a loop
    that starts over at the peeled round: each breaks 'exactly once, every fetch real' on some row"""
    caught = [row for row in ROWS if kc.defects(row, n_cu, mistake)]
    assert caught, mistake
    assert all(6 <= row.variant <= 8 for row in caught)          # the mistakes are in k_kq_lds's model only
    if mistake == "tail_first_slot_only":
        assert {row.variant for row in caught} == {8}            # PD = 2 has a tail of one at most
        assert any(row.kq_grid == 0 and row.L in (12, 14) and row.k == 5 for row in caught)     # the small tail-of-two rows
