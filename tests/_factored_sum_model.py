"""The factored form of the generator's tile sums (option sums_factored): a host restatement of its
classification, a numpy restatement of its order of arithmetic (built on _tile_sum_model, which keeps describing the
unfactored order: the fallback), and the programs tests/test_factored_sum_model.py (CPU) and
tests/test_gpu_factored_sums.py share.

Classification (flush_init_product_r).  A factor is tile-uniform when every qubit it touches is a block bit: no
register bit, no lane bit, neither wave bit.  The others are inner.  D = the block bits an inner factor touches, less
the zero qubits (a zero block bit is 0 wherever the sum is not).  The inner pass takes its group bits by the usual rule
(_tile_sum_model.choose_group_bits) among D, counting inner factors only.

Order.  inner(t restricted to D) is what k_prod_sums gives for the inner factors alone on the tile whose other
tile-index bits are 0; then, one thread per tile,
    tile_sums[t] = 0.0 where t hits a zero block bit, else inner x w_u(t) for the tile-uniform factors u in list order.

Rounding.  Unfactored, a thread's term is a product of nfac weights (2 ulp for w = fma(re, re, im im), 1 for its
multiply: 3 per factor) and the additions follow.  Factored, the inner factors' 3 ulp each enter before the addition
chain (R or 2^R, 6, 2: unchanged) and each tile-uniform factor's 3 ulp after it, as a multiply of the finished sum.
Relative errors of products and of sums of non-negative terms add to first order wherever they enter, and the numbers
of factors and of additions are those of the unfactored form, so a tile's sum keeps _tile_sum_model.bound:
(9 nfac + 2^R + 32) 2^-53 of the exact sum of the stored |amp|^2, nfac counting every factor.  A zero weight makes its
product 0 on either side of the sum: exact zeros stay exact."""
import numpy as np

import _tile_sum_model as tm
from _deferred_cases import random_factors, table


AUTO_MIN_BITS = 3          # sums_factored = -1 takes the factored launch from this many removed tile-index bits (measured: DESIGN §9)


def split(L, r, bit0, zero, factors):
    """(inner factor numbers, tile-uniform factor numbers, D as ascending block qubits)"""
    _, _, block = tm.geometry(L, r, bit0)
    uniform = [k for k, qs in enumerate(factors) if all(q in block for q in qs)]
    inner = [k for k in range(len(factors)) if k not in uniform]
    d = sorted({q for k in inner for q in factors[k] if q in block and q not in zero})
    return inner, uniform, d


def info(L, r, bit0, zero, factors, option=-1):
    """what Engine.tile_sums_info() reports"""
    _, _, block = tm.geometry(L, r, bit0)
    inner, uniform, d = split(L, r, bit0, zero, factors)
    need = {0: len(block) + 1, 1: 1, -1: AUTO_MIN_BITS}[option]
    return {"factored": len(block) - len(d) >= need, "d_bits": len(d), "inner": len(inner), "uniform": len(uniform)}


def inner_group_bits(L, r, bit0, zero, factors, want):
    regs, _, _ = tm.geometry(L, r, bit0)
    inner, _, d = split(L, r, bit0, zero, factors)
    return tm.choose_group_bits(L, regs, d, zero, [factors[k] for k in inner], want)


def model_factored_sums(L, r, bit0, want, zero, initval, factors, tables):
    """every tile's sum in the factored order (IEEE double operations as the two kernels do them)"""
    regs, thr, block = tm.geometry(L, r, bit0)
    inner, uniform, d = split(L, r, bit0, zero, factors)
    group = inner_group_bits(L, r, bit0, zero, factors, want)
    assert all(q in d for q in group)
    # the inner factors alone; the tile whose bits outside D are 0 is the one the inner pass visits
    full = tm.model_tile_sums(L, regs, thr, block, group, zero, initval, [factors[k] for k in inner],
                              [tables[k] for k in inner])
    dm = sum(1 << i for i, q in enumerate(block) if q in d)
    zm = sum(1 << i for i, q in enumerate(block) if q in zero)
    t = np.arange(1 << len(block), dtype=np.int64)
    out = full[t & dm]
    base = np.zeros_like(t)
    for i, q in enumerate(block):
        base |= ((t >> i) & 1) << q
    for k in uniform:
        out = out * tm.weights(tables[k])[tm._index(factors[k], base)]
    return np.where(t & zm, 0.0, out)


def tables_for(factors, seed, overrides=None):
    rs = np.random.RandomState(seed)
    out = []
    for i, qs in enumerate(factors):
        t = table(rs, len(qs))
        if overrides and i in overrides:
            t = np.asarray(overrides[i], dtype=np.complex128)
        out.append(t)
    return out


def numpy_state(w, zero, factors, tables):
    addr = np.arange(1 << w, dtype=np.int64)
    initval = 2.0 ** (-(w - len(zero)) / 2.0)
    amp = np.full(1 << w, initval, dtype=np.complex128)
    for q in zero:
        amp[(addr >> q) & 1 == 1] = 0.0
    for qs, t in zip(factors, tables):
        amp = amp * t[tm._index(qs, addr)]
    return amp, initval


# ---------------------------------------------------------------------------------------------------------------
# The programs.  W = 16, R = 4, init_prod_bit0 = -1: lane bits 0..4 and 11, wave bits 5 and 6, block bits 7..10 (16
# tiles), register bits 12..15.  W = 18 / 20 on the top bits: block bits 7..10, 12, 13 (, 14, 15): 64 / 256 tiles.
# A case: w, r, bit0, zero, factors, seed, overrides {factor: table}; claim = (|D|, inner, uniform) where the case is
# built to have it.
# ---------------------------------------------------------------------------------------------------------------
_INNER0 = [[0, 1], [3, 12], [5], [11, 13], [6, 2, 14]]
_UNI = [[7], [8, 9], [10, 7], [9]]


def case(w=16, r=4, bit0=-1, zero=(15,), factors=None, seed=1, overrides=None, claim=None):
    return dict(w=w, r=r, bit0=bit0, zero=list(zero), factors=factors, seed=seed, overrides=overrides, claim=claim)


def spread_case(w, r, bit0, seed, zero=None):
    """random inner factors, two block bits kept for tile-uniform factors where the geometry has them"""
    zero = [w - 1] if zero is None else zero
    _, _, block = tm.geometry(w, r, bit0)
    keep = [q for q in block if q not in zero][:2]
    fl = random_factors(w, zero + keep, 10, seed=seed)
    for q in keep:
        fl.insert(3, [q])
    if len(keep) == 2:
        fl.append(keep[::-1])
    return case(w, r, bit0, zero, fl, seed)


def _hundred():
    """98 factors that leave block bits 8 and 10 alone, a tile-uniform factor on each descriptor lane's range"""
    fl = random_factors(16, [15, 8, 10], 98, seed=2, kmax=3)
    fl.insert(3, [8])
    fl.insert(90, [10, 8])
    return fl


def _lds_limit():
    rs = np.random.RandomState(9)
    pool = [q for q in range(15) if q not in (8, 10)]           # block bits 8 and 10 stay outside D
    fl = [[int(q) for q in rs.choice(pool, size=k, replace=False)] for k in (10, 10, 8, 7, 6, 5)]
    fl += [[7, 8, 9, 10], [3, 9, 12], [8, 10]]
    assert sum(2 ** len(qs) for qs in fl) == 2556
    return fl


_ZERO_UNI = np.array([0.7, 0.0, 0.9j, 0.0])            # factor [8, 9]: zero where qubit 8 is set
_ZERO_IN = np.array([0.6, 1.1j, 0.0, 0.8])             # factor [7, 2]: zero where qubit 7 is clear and qubit 2 set

CASES = {
    "d0": case(factors=_INNER0 + _UNI, seed=1, claim=(0, 5, 4)),
    "d1": case(factors=_INNER0[:2] + _UNI[:2] + [[7, 2]] + _UNI[2:] + _INNER0[2:], seed=2, claim=(1, 6, 4)),
    "d2": case(factors=[[7, 2], [8], [9, 12], [10, 8]] + _INNER0, seed=3, claim=(2, 7, 2)),
    "d3": case(factors=[[7, 2], [8], [9, 12], [10, 5, 13], [8]] + _INNER0, seed=4, claim=(3, 8, 2)),
    "d4_no_uniform": case(factors=[[7, 2], [8, 0], [9, 12], [10, 5, 13]] + _INNER0, seed=5, claim=(4, 9, 0)),
    "only_uniform": case(factors=[[7], [8, 9], [10]], seed=6, claim=(0, 0, 3)),
    "w18": case(w=18, zero=(17,), factors=[[7, 1], [7, 8, 9, 10, 12, 13], [9, 14], [13, 3, 5], [8, 12], [0, 1], [3, 14], [5], [11, 15], [6, 2, 16]], seed=7,
                claim=(3, 8, 2)),
    "w20": case(w=20, zero=(19,), factors=[[7, 1], [7, 8, 9, 10, 12, 13, 14, 15], [9, 16], [13, 3, 5], [14, 10], [0, 1], [3, 16], [5], [11, 17],
                                                   [6, 2, 18]], seed=8, claim=(3, 8, 2)),
    "zero_uniform_entry": case(factors=[[7, 2], [8, 9], [3, 12], [10]] + _INNER0, seed=9, overrides={1: _ZERO_UNI},
                               claim=(1, 7, 2)),
    "zero_inner_entry": case(factors=[[7, 2], [8, 9], [3, 12], [10]] + _INNER0, seed=10, overrides={0: _ZERO_IN},
                             claim=(1, 7, 2)),
    "hundred": case(factors=_hundred(), seed=11),
    "lds_limit": case(factors=_lds_limit(), seed=12),
}
for _zq in (15, 3, 5, 9, 8, None):                     # register, lane, wave, block in D, block outside D, none
    CASES["zero_%s" % _zq] = case(zero=() if _zq is None else (_zq,),
                                  factors=[qs for qs in [[7, 2], [8, 10], [9, 12], [1, 13], [8]] + _INNER0
                                           if _zq not in qs or len(qs) > 1 and _zq in (8, 9)], seed=13)
for _r in (3, 4, 5, 6):
    for _b in (0, -1, 8):
        CASES["r%d_bit%d" % (_r, _b)] = spread_case(16, _r, _b, seed=20 + _r)
