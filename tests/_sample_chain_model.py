"""The sampler's walk over the super sums, twice in numpy doubles: as qsv_sample's host loop does it (sample_chain = 0)
and as k_walk_super / k_walk_shots do it on the device (sample_chain = 1).  Every operation is one IEEE double
operation in the order the source has it, so equal results here mean equal (block, residual) pairs there.

    total   pairwise_sum: runs of at most 64 entries summed left to right from 0, halves added
    r       min(raw * (total / run), nextafter(total, 0))
    host    b walks up while b < last_nz and r >= pre + bs[b], pre += bs[b]; (b, max(0, r - pre))
    device  P[b + 1] = P[b] + bs[b] by one thread; the first b with r < P[b + 1] by binary search over [0, last_nz]
"""
import numpy as np


def pairwise_sum(x):
    """qsv_measure.inc's recursion, word for word"""
    n = len(x)
    if n <= 64:
        s = 0.0
        for v in x:
            s = s + float(v)
        return s
    m = n // 2
    return pairwise_sum(x[:m]) + pairwise_sum(x[m:])


def device_total(x):
    """k_walk_super: leaves of 64 (one thread each), then adjacent partial sums added level by level; a power-of-two
    count"""
    n = len(x)
    assert n & (n - 1) == 0
    nc = 1 if n <= 64 else n // 64
    ln = n if n <= 64 else 64
    cs = []
    for t in range(nc):
        s = 0.0
        for i in range(ln):
            s = s + float(x[t * 64 + i])
        cs.append(s)
    st = 1
    while st < nc:
        for t in range(0, nc, 2 * st):
            cs[t] = cs[t] + cs[t + st]
        st *= 2
    return cs[0]


def last_nonzero(bs):
    last = 0
    for b, v in enumerate(bs):
        if v > 0:
            last = b
    return last


def uniforms(total, raw, run):
    """the shots' sorted positions in [0, total) from the running sums of the spacings"""
    scale = total / run
    cap = float(np.nextafter(total, 0.0))
    return [min(float(v) * scale, cap) for v in raw]


def host_walk(bs, r):
    """qsv_sample's loop over the sorted positions r (one shard: base = 0)"""
    last_nz = last_nonzero(bs)
    b, pre = 0, 0.0
    out = []
    for x in r:
        while b < last_nz and x >= pre + float(bs[b]):
            pre = pre + float(bs[b])
            b += 1
        out.append((b, max(0.0, x - pre)))
    return out


def device_walk(bs, r, clamp=True, strict=True):
    """k_walk_super's prefix and k_walk_shots' search.  clamp=False searches the whole array instead of [0, last_nz];
    strict=False compares r <= P[b + 1]: the two mistakes the tests must see."""
    n = len(bs)
    q = []
    pre = 0.0
    for v in bs:
        pre = pre + float(v)
        q.append(pre)
    last = last_nonzero(bs) if clamp else n - 1
    out = []
    for x in r:
        lo, hi = 0, last
        while lo < hi:
            mid = (lo + hi) >> 1
            if (x < q[mid]) if strict else (x <= q[mid]):
                hi = mid
            else:
                lo = mid + 1
        d = x - (q[lo - 1] if lo else 0.0)
        out.append((lo, d if 0.0 < d else 0.0))
    return out


def spacings(shots, seed):
    """running sums of shots + 1 exponentials: (raw[0..shots), run).  Any positive increasing sequence serves the
    model: the engine's come from mt19937_64, these from numpy."""
    rs = np.random.RandomState(seed)
    e = -np.log((rs.randint(0, 1 << 53, size=shots + 1, dtype=np.int64) + 1) * (1.0 / 9007199254740992.0))
    run = 0.0
    raw = []
    for v in e[:-1]:
        run = run + float(v)
        raw.append(run)
    run = run + float(e[-1])
    return raw, run
