"""The generator's tile geometry and a numpy restatement of k_prod_sums, shared by tests/test_tile_sum_model.py (CPU)
and tests/test_gpu_tile_sums.py.

Geometry (flush_init_product_r): R register bits from b0; 8 thread bits (6 lane bits, 2 wave bits); every other bit
of the shard's address is a block bit, and the tile index is the block bits compacted in ascending order.

The bound both tests hold a tile's sum to, relative to the exact sum of the stored |amp|^2 over the tile:
    (9 nfac + 2^R + 32) 2^-53
A stored amplitude is a product of nfac table entries: 3 ulp per complex multiply, twice for |stored|^2 = 6 nfac.
The kernel's term is a product of nfac weights w = fma(re, re, im * im): 2 ulp for the weight, 1 for its multiply =
3 nfac.  Additions of non-negative terms cost one ulp each along the longest chain: the register sum (R two-term
sums multiplied together, or a tree of R levels over 2^R terms: at most 2^R), the wave's tree (6 levels) and the four
waves (2 levels), with 32 for these and the init value's square."""
import math
from fractions import Fraction

import numpy as np


def bound(nfac, r):
    return (9 * nfac + 2 ** r + 32) * 2.0 ** -53


def geometry(L, r=0, bit0=0, lane_map=1):
    """(register bits, address of every thread index 0..255 within a tile, block bits ascending)"""
    top = bit0 < 0 or (bit0 == 0 and L >= 33)
    r = r or (4 if top else 5)
    b0 = 6
    if top:
        b0 = L - r
    elif bit0 > 6:
        b0 = min(bit0, L - r)
    regs = list(range(b0, b0 + r))
    if b0 == 6:
        lanepos = [3, 4, 6 + r]
    elif lane_map == 1 and b0 > 11 and L >= 14:
        lanepos = [3, 4, 11]
    else:
        lanepos = []
    free = [q for q in range(L) if q not in regs and q not in lanepos]       # ins_bits: values fill these in order
    nthr = 5 if lanepos else 8
    thr = np.zeros(256, dtype=np.int64)
    for t in range(256):
        u = ((t >> 6) << 3) | (t & 7) if lanepos else t
        a = 0
        for i in range(nthr):
            a |= ((u >> i) & 1) << free[i]
        for i, p in enumerate(lanepos):
            a |= ((t >> (3 + i)) & 1) << p
        thr[t] = a
    return regs, thr, free[nthr:]


def tile_index(addr, block_bits):
    t = np.zeros_like(addr)
    for i, q in enumerate(block_bits):
        t |= ((addr >> q) & 1) << i
    return t


def exact_tile_sums(amp, block_bits):
    """math.fsum of |amp|^2 over every tile's addresses (amp: one shard)"""
    p = amp.real.astype(np.float64) ** 2
    q = amp.imag.astype(np.float64) ** 2
    # re^2 and im^2 are rounded once each (half an ulp, inside the bound's 32); fsum adds them without further error
    t = tile_index(np.arange(amp.size, dtype=np.int64), block_bits)
    order = np.argsort(t, kind="stable")
    n = 1 << len(block_bits)
    pq = np.stack([p[order], q[order]], axis=1).reshape(n, -1)
    return np.array([math.fsum(row) for row in pq])


def choose_group_bits(L, regs, block_bits, zero, factors, want):
    """the host's rule: never a zero qubit; fewest factors first, then bits sharing no factor with a register bit, then
    the lowest; at most ``want`` (-1: 3) and never more than the tile index has"""
    want = min(3 if want < 0 else want, len(block_bits), 4)
    nfq, regq = [0] * L, [False] * L
    for qs in factors:
        reg = any(q in regs for q in qs)
        for q in qs:
            nfq[q] += 1
            regq[q] |= reg
    cand = sorted((q for q in block_bits if q not in zero), key=lambda q: (nfq[q], regq[q], q))
    return sorted(cand[:max(want, 0)])


def weights(table):
    """w = fma(re, re, im * im), rounded once"""
    t = np.asarray(table, dtype=np.complex128)
    return np.array([float(Fraction(float(z.real)) ** 2 + Fraction(float(z.imag) * float(z.imag))) for z in t])


def _index(qs, addr):
    j = np.zeros_like(addr)
    for e, q in enumerate(qs):
        j |= ((addr >> q) & 1) << e
    return j


def _tree(x):
    """pairwise over the last axis, neighbours first"""
    while x.shape[-1] > 1:
        x = x[..., 0::2] + x[..., 1::2]
    return x[..., 0]


def model_tile_sums(L, regs, thr, block_bits, group_bits, zero, initval, factors, tables):
    """every tile's sum as k_prod_sums forms it (IEEE double operations in the kernel's order; numpy contracts nothing)"""
    R = len(regs)
    nonmask = sum(1 << q for q in zero)
    W = [weights(t) for t in tables]
    cls = {"outer": [], "group": [], "multi": [], "mixed": []}
    single = [[] for _ in regs]
    for k, qs in enumerate(factors):
        nreg = [q for q in qs if q in regs]
        ngb = [q for q in qs if q in group_bits]
        if not nreg:
            cls["group" if ngb else "outer"].append(k)
        elif ngb:
            cls["mixed"].append(k)
        elif len(nreg) == 1:
            single[regs.index(nreg[0])].append(k)
        else:
            cls["multi"].append(k)
    regsum = bool(cls["multi"] or cls["mixed"])
    regaddr = np.array([sum(((j >> c) & 1) << regs[c] for c in range(R)) for j in range(1 << R)], dtype=np.int64)
    ntiles = 1 << len(block_bits)
    out = np.zeros(ntiles)
    gpos = [block_bits.index(q) for q in group_bits]
    gmask = sum(1 << p for p in gpos)
    for tile0 in range(ntiles):
        if tile0 & gmask:
            continue
        base = sum(((tile0 >> i) & 1) << q for i, q in enumerate(block_bits))
        if base & nonmask:
            continue                                   # the group's sums stay 0.0
        addr = base | thr
        w0 = np.where((thr & nonmask) == 0, initval * initval, 0.0)
        for k in cls["outer"]:
            w0 = w0 * W[k][_index(factors[k], addr)]
        N = np.ones(256)
        A = np.ones((256, 1))
        for c in range(R):
            t0 = np.ones(256)
            t1 = np.zeros(256) if (nonmask >> regs[c]) & 1 else np.ones(256)
            for k in single[c]:
                t0 = t0 * W[k][_index(factors[k], addr)]
                if not (nonmask >> regs[c]) & 1:
                    t1 = t1 * W[k][_index(factors[k], addr | (1 << regs[c]))]
            if regsum:
                A = np.concatenate([A * t0[:, None], A * t1[:, None]], axis=1)     # j | (1 << c) follows j
            else:
                N = N * (t0 + t1)
        if regsum:
            for k in cls["multi"]:
                A = A * W[k][_index(factors[k], addr[:, None] | regaddr[None, :])]
            if not cls["mixed"]:
                N = _tree(A)
        for b in range(1 << len(gpos)):
            ga = sum(1 << group_bits[i] for i in range(len(gpos)) if (b >> i) & 1)
            v = w0
            for k in cls["group"]:
                v = v * W[k][_index(factors[k], addr | ga)]
            if cls["mixed"]:
                T = A
                for k in cls["mixed"]:
                    T = T * W[k][_index(factors[k], (addr | ga)[:, None] | regaddr[None, :])]
                v = v * _tree(T)
            else:
                v = v * N
            x = v.reshape(4, 64)
            x = x[:, :32] + x[:, 32:]                  # lane l + lane l ^ 32
            x = x[:, :16] + x[:, 16:]                  # + lane l ^ 16
            w = _tree(x)                               # l ^ 1, l ^ 2, mirrored half row, mirrored row
            tile = tile0 | sum(1 << gpos[i] for i in range(len(gpos)) if (b >> i) & 1)
            out[tile] = (w[0] + w[1]) + (w[2] + w[3])
    return out


def engine_total(tile_sums):
    """one shard's mass as qsv_norm forms it from its tile sums (k_supersum, then the host's pairwise sum)"""
    n = tile_sums.size
    supers = []
    for lo in range(0, n, 1024):
        s = np.zeros(256)
        for k in range(4):
            part = tile_sums[lo + k * 256: min(lo + (k + 1) * 256, n)]
            s[:part.size] = s[:part.size] + part
        v = s.reshape(4, 64)
        lane = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            v = v + v[:, lane ^ o]
        supers.append((v[0, 0] + v[1, 0]) + (v[2, 0] + v[3, 0]))

    def pairwise(x):
        if len(x) <= 64:
            s = 0.0
            for y in x:
                s += y
            return s
        m = len(x) // 2
        return pairwise(x[:m]) + pairwise(x[m:])
    return pairwise(supers)
