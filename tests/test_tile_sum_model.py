"""CPU: the numpy restatement of k_prod_sums (_tile_sum_model.model_tile_sums: IEEE double operations in the kernel's
order) against math.fsum of |amp|^2 of the amplitudes numpy forms, within the bound the GPU test holds the kernel
to (_tile_sum_model.bound: its derivation is there).  So the bound is known to hold for the reference alone, on the
tests' tables (magnitudes 0.5 .. 1.5)."""
import numpy as np
import pytest

import _tile_sum_model as tm
from _deferred_cases import random_factors, table

W = 16


def _case(nfac, r, bit0, want, zero, seed, factors=None):
    rs = np.random.RandomState(seed)
    factors = factors or random_factors(W, zero, nfac, seed=seed, kmax=3 if nfac > 50 else 4)
    tables = [table(rs, len(qs)) for qs in factors]
    regs, thr, block = tm.geometry(W, r, bit0)
    group = tm.choose_group_bits(W, regs, block, zero, factors, want)
    initval = 2.0 ** (-(W - len(zero)) / 2.0)
    got = tm.model_tile_sums(W, regs, thr, block, group, zero, initval, factors, tables)
    addr = np.arange(1 << W, dtype=np.int64)
    amp = np.full(1 << W, initval, dtype=np.complex128)
    for q in zero:
        amp[(addr >> q) & 1 == 1] = 0.0
    for qs, t in zip(factors, tables):
        amp = amp * t[tm._index(qs, addr)]
    want_sums = tm.exact_tile_sums(amp, block)
    rel = tm.bound(len(factors), len(regs))
    err = np.abs(got - want_sums)
    assert (err <= rel * want_sums).all(), float((err / np.where(want_sums > 0, want_sums, 1)).max()) / rel
    assert (got[want_sums == 0.0] == 0.0).all()
    return float((err / np.where(want_sums > 0, want_sums, 1)).max()) / rel


@pytest.mark.parametrize("nfac", [14, 100])
@pytest.mark.parametrize("r,bit0,want", [(4, -1, -1), (4, -1, 0), (5, 0, 4), (3, 8, 2), (6, -1, 1)])
def test_model_within_the_bound(nfac, r, bit0, want):
    _case(nfac, r, bit0, want, [15], seed=nfac + r)


@pytest.mark.parametrize("zq", [15, 3, 5, 9])
def test_model_with_a_zero_qubit(zq):
    _case(16, 4, -1, -1, [zq], seed=zq)


def test_model_multi_and_mixed_factors():
    fl = [[7, 12], [9, 13, 14], [8, 10, 12, 13], [3], [12, 13], [12, 14, 3], [13, 14, 8, 0], [12, 13, 14]]
    _case(len(fl), 4, -1, 4, [15], seed=1, factors=fl)


def test_geometry_of_the_documented_tile():
    """W = 16, R = 4 on the top bits: lane bits 0..4 and 11, wave bits 5 and 6, block bits 7..10, registers 12..15"""
    regs, thr, block = tm.geometry(16, 4, -1)
    assert regs == [12, 13, 14, 15] and block == [7, 8, 9, 10]
    assert sorted(int(a) for a in thr[:64]) == sorted(sum(((l >> i) & 1) << q for i, q in enumerate([0, 1, 2, 3, 4, 11])) for l in range(64))
    assert int(thr[64]) == 1 << 5 and int(thr[128]) == 1 << 6
    assert len(set(thr.tolist())) == 256
