"""The shard-bit exchange between virtual shards of one process, case by case against the exact permutation
(_exchange_cases.py): both forms of k_swap_blocks (plain and with the index swizzle, which ``swizzle`` 2 selects from
2^14 amplitudes per shard on), every position of the swapped local bits that decides between them, pair order against
shard-bit order, one-block shards, and sequences compared after every step.  The states encode their index, so equality is
exact and a failure names the index it found.  test_gpu_multiproc_exact.py runs the same table between rank processes."""
import numpy as np
import pytest

import _exchange_cases as xc

pytestmark = pytest.mark.gpu

SWIZZLES = (0, 2)


@pytest.fixture(scope="module")
def lib():
    from qcmrf_amd import _lib
    _lib.load()
    assert _lib.device_count() >= 1
    return _lib


SHAPES = sorted({(c.W, c.P) for c in xc.all_cases()})


@pytest.mark.parametrize("W,P", SHAPES)
def test_every_case_under_both_swizzle_settings(lib, W, P):
    cases = [c for c in xc.all_cases() if (c.W, c.P) == (W, P)]
    state = xc.encode_state(W)
    got = {}
    with lib.Engine(W, devices=(0,) * P) as eng:
        for swz in SWIZZLES:
            eng.set_option("swizzle", swz)
            for c in cases:
                eng.set_amplitudes(0, state)
                eng.reset_stats()
                eng.swap_layout(c.a, c.b)
                out = eng.amplitudes()
                want = xc.expected_state(c.name)
                assert np.array_equal(out, want), (c.name, swz, xc.first_mismatch(out, want))
                assert eng.stats()["exchanges"] == c.exchanges, (c.name, swz)
                got[c.name, swz] = out
    for c in cases:
        assert got[c.name, 0].tobytes() == got[c.name, 2].tobytes(), c.name             # bit for bit, signs of zeros included


@pytest.mark.parametrize("name", sorted(xc.SEQUENCES))
def test_sequences_step_by_step(lib, name):
    W, P, steps = xc.SEQUENCES[name]
    want = xc.sequence_states(name)
    counts = xc.sequence_exchanges(name)
    seen = {}
    with lib.Engine(W, devices=(0,) * P) as eng:
        for swz in SWIZZLES:
            eng.set_option("swizzle", swz)
            eng.set_amplitudes(0, xc.encode_state(W))
            eng.reset_stats()
            for k, st in enumerate(steps):
                if st[0] == "swap":
                    eng.swap_layout(st[1], st[2])
                else:
                    eng.apply_1q(st[1], st[2])
                out = eng.amplitudes()
                assert np.array_equal(out, want[k]), (name, swz, k, xc.first_mismatch(out, want[k]))
                assert eng.stats()["exchanges"] == sum(counts[:k + 1]), (name, swz, k)
                seen[swz, k] = out
    for k in range(len(steps)):
        assert np.array_equal(seen[0, k], seen[2, k]), (name, k)
