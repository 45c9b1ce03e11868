"""Exact host reference of ``qsv_sample`` (test infrastructure; numpy and ``math`` only): which uniform drew which word.

``qsv_sample`` is deterministic given (state, seed, shots):

  1. ``std::mt19937_64(seed)`` yields ``shots + 1`` exponential spacings ``-log(((x >> 11) + 1) * 2^-53)``; their
     running sums, scaled by ``total / (sum of all shots + 1)`` and clamped to ``nextafter(total, 0)``, are the uniforms
     ``r[0] <= r[1] <= ...`` in ``[0, total)`` -- already sorted (order statistics of iid uniforms);
  2. shot ``s`` takes the index at which an inverse-CDF walk over |amp|^2 crosses ``r[s]``: in ascending index order when
     the sampler reads the amplitudes itself, in the tile order of the program's last pass when that pass left its
     per-tile sums behind;
  3. the same generator then shuffles the words (Fisher-Yates, ``k = rng() % (s + 1)`` for ``s = shots-1 .. 1``).

So a test can rebuild ``r``, undo the shuffle, and hold every word against the uniform that produced it:

  MT64                 mt19937_64, output-exact (the recurrence and tempering the C++ standard fixes)
  sorted_uniforms      step 1, the same expression sequence in the same order (``math.log`` is the C library's ``log``)
  unshuffle            step 3 inverted: ``x[s]`` is the word drawn for ``r[s]``
  exact_index_order    step 2 in ascending index order, prefix sums in ``longdouble``; and each shot's distance to the
                       nearest prefix boundary (a shot closer than the tolerance may legitimately fall on either side)
  check_inverse_cdf    the contract every inverse-CDF walk over ANY fixed order of the indices satisfies: no knowledge
                       of tiles, X frames or implied zeros needed
  model_sampler        numpy inverse CDF over a given order (host tests and their mutations)

Tolerance.  ``TOL_REL = 1e-12`` of the total mass, derived, not measured.  Every quantity compared here is a sum of at
most 2^W non-negative doubles that the sampler and the reference add in different orders.  A chain of k sequential
additions of non-negative terms is off by at most k * 2^-53 of its result.  The chains of the sampler: the host's
walk over block sums (2^(W-12) of them) or super sums (fewer), 64 rows plus a 6-step scan in k_locate, 16 rows plus 6
in k_locate_super, 2^R + 6 + 4 <= 74 in k_locate_tile, and the sum trees (a few dozen levels in all): fewer than
2^(W-12) + 200 additions on any path.  At W <= 23 that is 2248 * 1.1e-16 < 2.5e-13 of the total, so 1e-12 leaves a
factor of 4.  It does not move with what a run shows.
"""
from __future__ import annotations

import math

import numpy as np

TOL_REL = 1e-12

_NN, _MM = 312, 156
_MATRIX_A = 0xB5026F5AA96619E9
_UM, _LM = 0xFFFFFFFF80000000, 0x7FFFFFFF
_M64 = (1 << 64) - 1


class MT64:
    """mt19937_64: ``MT64(seed)()`` returns what ``std::mt19937_64(seed)()`` returns, call for call."""

    def __init__(self, seed):
        mt = [0] * _NN
        mt[0] = int(seed) & _M64
        for i in range(1, _NN):
            mt[i] = (6364136223846793005 * (mt[i - 1] ^ (mt[i - 1] >> 62)) + i) & _M64
        self._mt = np.array(mt, dtype=np.uint64)
        self._out = np.empty(0, dtype=np.uint64)
        self._pos = 0

    def _twist(self):
        mt = self._mt
        um, lm, a, one = np.uint64(_UM), np.uint64(_LM), np.uint64(_MATRIX_A), np.uint64(1)

        def step(cur, nxt, far):
            x = (cur & um) | (nxt & lm)
            return far ^ (x >> one) ^ ((x & one) * a)
        # in-place recurrence: word i reads words i, i + 1 (not yet rewritten) and i + 156 mod 312 (rewritten from i = 156 on)
        mt[:_NN - _MM] = step(mt[:_NN - _MM], mt[1:_NN - _MM + 1], mt[_MM:])
        mt[_NN - _MM:_NN - 1] = step(mt[_NN - _MM:_NN - 1], mt[_NN - _MM + 1:], mt[:_MM - 1])
        mt[_NN - 1] = step(mt[_NN - 1], mt[0], mt[_MM - 1])
        y = mt.copy()
        y ^= (y >> np.uint64(29)) & np.uint64(0x5555555555555555)
        y ^= (y << np.uint64(17)) & np.uint64(0x71D67FFFEDA60000)
        y ^= (y << np.uint64(37)) & np.uint64(0xFFF7EEE000000000)
        y ^= y >> np.uint64(43)
        return y

    def draw(self, n):
        """the next ``n`` outputs as a uint64 array"""
        n = int(n)
        parts = []
        while n > 0:
            if self._pos == len(self._out):
                self._out = self._twist()
                self._pos = 0
            take = min(n, len(self._out) - self._pos)
            parts.append(self._out[self._pos:self._pos + take])
            self._pos += take
            n -= take
        return np.concatenate(parts) if parts else np.empty(0, dtype=np.uint64)

    def __call__(self):
        return int(self.draw(1)[0])


def _spacings(rng, count):
    """-log(((x >> 11) + 1) * 2^-53) per draw: the integer is at most 2^53 and the scaling a power of two, so the
    argument of the logarithm is exact"""
    x = (rng.draw(count) >> np.uint64(11)).astype(np.int64) + 1
    return [-math.log(float(v) * (1.0 / 9007199254740992.0)) for v in x.tolist()]


def sorted_uniforms(seed, shots, total, rng=None):
    """r[0..shots) of ``qsv_sample(shots, seed)`` on a state of mass ``total`` (float64 array).  ``rng``: a fresh
    ``MT64(seed)`` to draw from, left where the sampler's generator stands before its shuffle."""
    shots = int(shots)
    total = float(total)
    rng = MT64(seed) if rng is None else rng
    e = _spacings(rng, shots + 1)
    r = np.empty(shots, dtype=np.float64)
    run = 0.0
    for s in range(shots):
        run += e[s]
        r[s] = run
    run += e[shots]
    scale = total / run
    return np.minimum(r * scale, math.nextafter(total, 0.0))


def shuffle_swaps(seed, shots):
    """(s, k) pairs of the sampler's final Fisher-Yates pass, in the order it performs them"""
    shots = int(shots)
    rng = MT64(seed)
    rng.draw(shots + 1)
    if shots < 2:
        return np.empty(0, dtype=np.int64), np.empty(0, dtype=np.int64)
    s = np.arange(shots - 1, 0, -1, dtype=np.uint64)
    k = rng.draw(shots - 1) % (s + np.uint64(1))
    return s.astype(np.int64), k.astype(np.int64)


def unshuffle(seed, shots, words):
    """undo the sampler's shuffle: returns x with x[s] the word drawn for r[s]"""
    x = np.array(words, copy=True)
    if len(x) != int(shots):
        raise ValueError("%d words for %d shots" % (len(x), int(shots)))
    s, k = shuffle_swaps(seed, shots)
    xl = x.tolist()
    for a, b in zip(s[::-1].tolist(), k[::-1].tolist()):       # the swaps are involutions: replay them backwards
        xl[a], xl[b] = xl[b], xl[a]
    return np.array(xl, dtype=x.dtype)


def exact_index_order(p, r):
    """(index, distance) per shot: the first index i with p[i] > 0 whose inclusive prefix sum (longdouble, ascending
    global index) exceeds r[s]; the last such index if there is none.  distance[s] is how far r[s] lies from the
    nearest boundary between two populated indices (inf where the state has a single one)."""
    p = np.asarray(p, dtype=np.float64)
    r = np.asarray(r, dtype=np.float64)
    sup = np.flatnonzero(p > 0)
    if sup.size == 0:
        raise ValueError("state has no mass")
    cum = np.cumsum(p[sup].astype(np.longdouble))             # inclusive prefix over the populated indices only
    rl = r.astype(np.longdouble)
    pos = np.searchsorted(cum, rl, side="right")               # first populated position with cum > r
    pos = np.minimum(pos, sup.size - 1)
    inner = cum[:-1]                                           # the boundaries a shot could fall on either side of
    if inner.size == 0:
        dist = np.full(r.shape, np.inf)
    else:
        j = np.searchsorted(inner, rl, side="left")
        lo = np.where(j > 0, rl - inner[np.maximum(j - 1, 0)], np.inf)
        hi = np.where(j < inner.size, inner[np.minimum(j, inner.size - 1)] - rl, np.inf)
        dist = np.minimum(lo, hi).astype(np.float64)
    return sup[pos].astype(np.uint64), dist


def model_sampler(p, order, r):
    """inverse CDF over the indices in ``order`` (a permutation of range(len(p))): per shot the first index of the
    walk with p > 0 whose running sum exceeds r[s], the walk's last populated index if none"""
    p = np.asarray(p, dtype=np.float64)
    order = np.asarray(order, dtype=np.int64)
    keep = order[p[order] > 0]
    cum = np.cumsum(p[keep].astype(np.longdouble))
    pos = np.minimum(np.searchsorted(cum, np.asarray(r).astype(np.longdouble), side="right"), keep.size - 1)
    return keep[pos].astype(np.uint64)


RULES = ("runs", "support", "upper", "lower", "prefix", "suffix")


def check_inverse_cdf(p, r, x, tol, total=None):
    """Violations of the layout-independent sampling contract, as a list of (rule, count, first shot).

    An inverse-CDF walk over some fixed order of the indices gives index i the interval [c_i, c_i + p_i) of [0, total),
    c_i the mass of the indices before it in that order.  With r sorted, whatever the order:

      runs     every distinct index occupies one contiguous run [a, b] of shots
      support  p[x[s]] > 0
      upper    r[b] - r[a] < p_i + tol                       both ends lie inside the interval
      lower    r[b+1] - r[a-1] > p_i - tol                   the neighbours lie outside it (r[-1] = 0, r[shots] = total)
      prefix   sum of p over the indices of earlier runs <= r[a] + tol      they all precede i in the walk
      suffix   sum of p over the indices of later runs <= total - r[b] + tol

    ``total``: the mass r was scaled to (default: fsum(p))."""
    p = np.asarray(p, dtype=np.float64)
    r = np.asarray(r, dtype=np.float64)
    x = np.asarray(x).astype(np.int64)
    total = math.fsum(p.tolist()) if total is None else float(total)
    shots = len(x)
    if len(r) != shots:
        raise ValueError("%d uniforms for %d words" % (len(r), shots))
    out = []

    def report(rule, bad, where):
        bad = np.asarray(bad)
        if bad.any():
            out.append((rule, int(bad.sum()), int(np.asarray(where)[np.flatnonzero(bad)[0]])))
    if shots == 0:
        return out
    if (x < 0).any() or (x >= p.size).any():
        out.append(("support", int(((x < 0) | (x >= p.size)).sum()), int(np.flatnonzero((x < 0) | (x >= p.size))[0])))
        return out
    a = np.concatenate(([0], np.flatnonzero(x[1:] != x[:-1]) + 1))        # first shot of every run
    b = np.concatenate((a[1:] - 1, [shots - 1]))                          # last shot
    ids = x[a]
    order = np.argsort(ids, kind="stable")
    again = np.zeros(len(ids), dtype=bool)
    again[order[1:]] = ids[order[1:]] == ids[order[:-1]]                  # a later run of an index already seen
    report("runs", again, a)
    report("support", ~(p[x] > 0), np.arange(shots))
    pi = p[ids].astype(np.longdouble)
    rl = r.astype(np.longdouble)
    ext = np.concatenate(([np.longdouble(0)], rl, [np.longdouble(total)]))    # ext[s + 1] = r[s]
    report("upper", ~(rl[b] - rl[a] < pi + tol), a)
    report("lower", ~(ext[b + 2] - ext[a] > pi - tol), a)
    before = np.concatenate(([np.longdouble(0)], np.cumsum(pi)[:-1]))
    after = np.cumsum(pi[::-1])[::-1] - pi
    report("prefix", ~(before <= rl[a] + tol), a)
    report("suffix", ~(after <= np.longdouble(total) - rl[b] + tol), a)
    return out


def rules_of(violations):
    return sorted(set(v[0] for v in violations))
