"""Post-selected sampling (``qsv_sample_cond``): the exact host reference, numpy restatements of the engine's two index
maps, and the stand-in engine of the host tests.  TEST INFRASTRUCTURE ONLY; written from the contract in include/qsv.h.

The contract is ``qsv_sample``'s (``_sampler_reference``) applied to the matching states: ``std::mt19937_64(seed)``
draws ``shots + 1`` spacings, the uniforms are scaled to the CONDITIONAL mass, the inverse-CDF walk runs in ascending
global index over the states g with ``(g & fix_mask) == fix_val``, the same Fisher-Yates shuffle follows.

  conditional_reference   (want, dist, r, mass): the word of every uniform, its distance to the nearest prefix boundary
  shuffled                the words in the order the engine returns them (the shuffle applied)
  compact_addresses       ``ins_bits(j, F) | val`` for j = 0 .. 2^(bits - |F|): the compact index space of the kernels
  tile_geometry / tile_list   the generator's tile map and the host's list of the tiles that hold the matching sub-cube
  CondNumpyEngine         ``oracle.sharded_numpy.NumpyEngine`` plus ``sample_cond`` (exact words) and ``state_info``
"""
from __future__ import annotations

import math

import numpy as np

from _sampler_reference import exact_index_order, shuffle_swaps, sorted_uniforms
from oracle.sharded_numpy import NumpyEngine


def match_of(size, fix_mask, fix_val):
    g = np.arange(size, dtype=np.uint64)
    return (g & np.uint64(fix_mask)) == np.uint64(fix_val)


def conditional_reference(p, fix_mask, fix_val, seed, shots, total=None):
    """per uniform r[s] (ascending) the index drawn, its distance to the nearest prefix boundary of the masked p, the
    uniforms, and the mass they were scaled to (``total``: the engine's own mass; default fsum of the masked p)"""
    p = np.asarray(p, dtype=np.float64)
    pm = np.where(match_of(p.size, fix_mask, fix_val), p, 0.0)
    mass = math.fsum(pm.tolist()) if total is None else float(total)
    if not mass > 0:
        raise ValueError("post-selected outcome has zero probability")
    r = sorted_uniforms(seed, shots, mass)
    want, dist = exact_index_order(pm, r)
    return want, dist, r, mass


def shuffled(seed, words):
    """the sampler's final Fisher-Yates pass applied to the words in uniform order"""
    x = np.array(words, copy=True).tolist()
    s, k = shuffle_swaps(seed, len(x))
    for a, b in zip(s.tolist(), k.tolist()):
        x[a], x[b] = x[b], x[a]
    return np.array(x, dtype=np.uint64)


# ---- the compact index space (BitIns / ins_bits of qsv_common.h) ---------------------------------------------------------
def ins_bits(x, positions):
    """a zero bit inserted at every position of ``positions`` (ascending), as the device helper does"""
    x = np.asarray(x, dtype=np.uint64).copy()
    for pos in sorted(positions):
        lo = x & np.uint64((1 << pos) - 1)
        x = ((x >> np.uint64(pos)) << np.uint64(pos + 1)) | lo
    return x


def compact_addresses(bits, fixed, val):
    """address of compact index j for every j: ``ins_bits(j, F) | val`` (val: the fixed bits' values, in place)"""
    j = np.arange(1 << (bits - len(fixed)), dtype=np.uint64)
    return ins_bits(j, fixed) | np.uint64(val)


# ---- the generator's tiles (qsv_multi.inc: flush_init_product_r; qsv_kmulti.h: tile_base_blk / tile_base_thr) -----------
class TileGeometry:
    """W local qubits, R register bits at ``reg``, lane bits 3..5 of a wave on ``lane3`` (None: the plain map).  A tile
    is 256 threads x 2^R amplitudes; ``ins`` lists the address bits the tile index does not count through."""

    def __init__(self, w, reg, lane3):
        self.w, self.reg, self.lane3 = w, list(reg), lane3
        self.ins = sorted(self.reg + (list(lane3) if lane3 is not None else []))
        self.ntiles = (1 << (w - len(self.reg))) // 256

    def base_blk(self, t):
        t = np.asarray(t, dtype=np.uint64)
        return ins_bits(t * np.uint64(256) if self.lane3 is None else t << np.uint64(5), self.ins)

    def block_bits(self):
        """address bit of tile-index bit b, for every b"""
        out = []
        b = 0
        while (1 << b) < self.ntiles:
            out.append(int(self.base_blk(1 << b)).bit_length() - 1)
            b += 1
        return out

    def tile_of(self, addr):
        """the tile every address belongs to"""
        addr = np.asarray(addr, dtype=np.uint64)
        t = np.zeros(addr.shape, dtype=np.uint64)
        for b, a in enumerate(self.block_bits()):
            t |= ((addr >> np.uint64(a)) & np.uint64(1)) << np.uint64(b)
        return t


def deferred_geometry():
    """_deferred_cases: W = 16, R = 4 on bits 12..15, lane bits 0..4 and 11, wave bits 5 and 6, block bits 7..10"""
    return TileGeometry(16, [12, 13, 14, 15], (3, 4, 11))


def tile_list(geo, fix_mask, fix_val):
    """the host's list (cond_prepare_deferred): the free tile-index bits counted up, the fixed ones deposited"""
    fixed, tval = [], 0
    for b, a in enumerate(geo.block_bits()):
        if (fix_mask >> a) & 1:
            fixed.append(b)
            tval |= ((fix_val >> a) & 1) << b
    j = np.arange(geo.ntiles >> len(fixed), dtype=np.uint64)
    return ins_bits(j, fixed) | np.uint64(tval), len(fixed)


# ---- the stand-in engine -------------------------------------------------------------------------------------------
class CondNumpyEngine(NumpyEngine):
    """NumpyEngine with the post-selected sampler, word-exact by the contract, and the state_info the backend reads"""

    def state_info(self):
        return {"deferred": False, "realize_calls": 0, "listed_launches": 0}

    def sample_cond(self, shots, seed, meas_qubits=None, fix_mask=0, fix_val=0):
        if fix_val & ~fix_mask or fix_mask >> self.n_qubits:
            raise ValueError("bad mask")
        owned = sorted(self.sh)
        assert owned == list(range(self.world)), "one process"
        p = np.concatenate([np.abs(self.sh[s]) ** 2 for s in owned])
        pm = np.where(match_of(p.size, fix_mask, fix_val), p, 0.0)
        mass = math.fsum(pm.tolist())
        if shots == 0:
            return np.zeros(0, dtype=np.uint64), mass
        want, _, _, _ = conditional_reference(p, fix_mask, fix_val, seed, shots)
        pick = shuffled(seed, want)
        if meas_qubits is None:
            return pick, mass
        out = np.zeros(shots, dtype=np.uint64)
        for b, q in enumerate(meas_qubits):
            if q >= 0:
                out |= ((pick >> np.uint64(q)) & np.uint64(1)) << np.uint64(b)
        return out, mass


def factory(n, devices=(0,), rank=None, world_size=None):
    return CondNumpyEngine(n, len(devices))
