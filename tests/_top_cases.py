"""The k most probable states of a conditioned state (``qsv_top_cond``): the exact host reference, the state builders and
masks the host and the GPU tests share, a block-wise selection with planted mistakes, and the stand-in engine of the host
tests.  TEST INFRASTRUCTURE ONLY; written from the contract in include/qsv.h, not from the kernel.

  top_reference     (indices uint64, p float64): p = re*re + im*im in float64 over the matching global indices, a stable
                    sort by (-p, index), entries whose p is not > 0 dropped, cut at k; ``hi`` is the global index of
                    amps[0] (a shard's amplitudes: hi = shard << L)
  builders          random / ascending / descending / sawtooth / two_maxima / equal_maxima / tiny_weights: the states of
                    tests/test_gpu_top_states.py
  MASKS             the 14-qubit fix sets of the GPU tests
  CASES             (name, amplitudes, k, fixed, hi): every planted mistake of tests/test_top_cases.py fails at least one
  top_planted       a block-wise selection (lists per block of candidates, threshold, merge), right or with one mistake
  TopNumpyEngine    ``MarginalsNumpyEngine`` plus ``top_cond`` by the reference, with the entry point's refusals
  MODELS            the (graph, seed of theta) pairs of the QCMRF-level tests; gaps_ok is their condition
"""
from __future__ import annotations

import numpy as np

import _sampler_cases as sc
from _marginal_cases import MarginalsNumpyEngine, mask_of   # noqa: F401  (mask_of: re-exported)

MAX_K = 64
N = 14
BLOCK = 4096               # compact entries per block


def weights(amps):
    """p = re*re + im*im, each operation rounded (no fused contraction): the weight of the contract"""
    a = np.asarray(amps, dtype=np.complex128)
    return a.real * a.real + a.imag * a.imag


def top_reference(amps, k, fix_mask, fix_val, hi=0):
    p = weights(amps)
    g = np.arange(p.size, dtype=np.uint64) + np.uint64(hi)
    sel = np.flatnonzero((g & np.uint64(fix_mask)) == np.uint64(fix_val))
    pm, gm = p[sel], g[sel]                                  # ascending index
    with np.errstate(invalid="ignore"):
        order = np.argsort(-pm, kind="stable")               # stable: equal p keep ascending index
        order = order[pm[order] > 0]                         # a 0 and a NaN are not > 0
    order = order[:k]
    return gm[order].astype(np.uint64), pm[order].astype(np.float64)


# ---- state builders (complex128, 2^w entries; not normalised: the entry point does not ask for it) ------------------------------
def random_state(w, seed):
    return sc.rand_state(w, seed)


def ascending(w):
    """p strictly ascending in the index: every block brings entrants"""
    return ((np.arange(1 << w, dtype=np.float64) + 1.0) / (1 << w)).astype(np.complex128)


def descending(w):
    return ascending(w)[::-1].copy()


def sawtooth(w, block=BLOCK):
    """p ascending within blocks of ``block`` entries and descending across them"""
    i = np.arange(1 << w, dtype=np.int64)
    nb = max(1, (1 << w) // block)
    v = (nb - 1 - i // block) * block + (i % block) + 1
    return (v.astype(np.float64) / (1 << w)).astype(np.complex128)


def background(w, seed, scale=0.3):
    rs = np.random.RandomState(seed)
    return scale * (rs.rand(1 << w) - 0.5) + 1j * scale * (rs.rand(1 << w) - 0.5)     # p <= 2 * 0.15^2 < 0.05


def two_maxima(w, j, t, seed=3):
    """two equal maxima at j and j ^ (1 << t) (one on the real, one on the imaginary axis: the same p) and a third,
    smaller entry; returns (amplitudes, the three indices in the order they must come back)"""
    a = background(w, seed + t)
    lo, hi = sorted((j, j ^ (1 << t)))
    third = (j + 5 * (1 << t) + 77) % (1 << w)
    while third in (lo, hi):
        third = (third + 1) % (1 << w)
    a[lo], a[hi], a[third] = 1.0, -1.0j, 0.875
    return a, [lo, hi, third]


def equal_maxima(w, count, seed=9):
    """``count`` equal maxima at random places over a smaller background; returns (amplitudes, their indices ascending)"""
    a = background(w, seed)
    at = np.sort(np.random.RandomState(seed).choice(1 << w, size=count, replace=False))
    a[at] = 1.0
    return a, at.astype(np.uint64)


def tiny_weights(w):
    """all zero but: two ordinary entries, one amplitude 1e-160 (p = 1e-320, a denormal) and amplitudes whose square
    underflows to 0; returns (amplitudes, the indices that must come back, in order)"""
    a = np.zeros(1 << w, dtype=np.complex128)
    n = 1 << w
    a[n - 3], a[5], a[n // 2 + 1] = 0.5, 0.25j, 1e-160
    a[7], a[n // 2 + 2], a[n - 1] = 1e-170, 1e-200j, 1e-170 + 1e-170j
    assert weights(a)[n // 2 + 1] > 0 and weights(a)[7] == 0.0 and weights(a)[n - 1] == 0.0
    return a, [n - 3, 5, n // 2 + 1]


# ---- the 14-qubit masks of the GPU tests: local bits 0..5 lane, 6..7 wave, 8..11 the thread's loads, 12.. the block -------------
F10 = {q: (q * 7 + 2) % 3 % 2 for q in range(10)}                     # 16 candidates: fewer than a block, fewer than k = 17
MASKS = {
    "none": {},
    "lane_bit": {3: 1},
    "wave_bit": {6: 0},
    "register_bit": {9: 1},
    "block_bit": {13: 1},
    "mixed": {2: 1, 7: 0, 10: 1, 12: 0},
    "ten_bits": F10,
}
KS = [1, 2, 17, 64]


# ---- a block-wise selection, right or with one planted mistake ------------------------------------------------------------------
MISTAKES = ["ties_descending_index", "ge_threshold", "zero_returned", "hi_dropped", "merged_unsorted"]


def top_planted(amps, k, fix_mask, fix_val, hi=0, mistake=None, block=16):
    """Lists of k per block of ``block`` candidates, each kept under a threshold (the weakest of a full list) while the
    candidates arrive in ascending index, then merged.  mistake None is the contract."""
    p = weights(amps)
    local = np.arange(p.size, dtype=np.int64)
    g = local + hi
    sel = np.flatnonzero((g & fix_mask) == fix_val)
    report = local if mistake == "hi_dropped" else g
    key = (lambda c: (-c[0], -c[1])) if mistake == "ties_descending_index" else (lambda c: (-c[0], c[1]))
    lists = []
    for b0 in range(0, sel.size, block):
        lst = []
        for i in sel[b0:b0 + block]:
            c = (float(p[i]), int(report[i]))
            if not (c[0] > 0 or (mistake == "zero_returned" and c[0] == 0)):
                continue
            if len(lst) < k:
                lst.append(c)
            elif (c[0] >= lst[-1][0]) if mistake == "ge_threshold" else (c[0] > lst[-1][0]):
                lst[-1] = c                                         # the weakest makes room
            else:
                continue
            lst.sort(key=key)
        lists.append(lst)
    flat = [c for lst in lists for c in lst]
    if mistake != "merged_unsorted":
        flat.sort(key=key)
    flat = flat[:k]
    return np.array([c[1] for c in flat], dtype=np.uint64), np.array([c[0] for c in flat], dtype=np.float64)


def _few_positive():
    a = np.zeros(64, dtype=np.complex128)
    a[9], a[41], a[43] = 0.5, 0.25j, 0.75
    return a


def _uniform(bits):
    return np.full(1 << bits, 0.125 + 0.125j)


# (name, amplitudes, k, fixed, hi)
CASES = [
    ("random", random_state(6, 5), 5, {}, 0),
    ("random_masked", random_state(7, 6), 4, {1: 1, 5: 0}, 0),
    ("two_equal_maxima", two_maxima(6, 21, 3)[0], 3, {}, 0),             # the order of a tie
    ("all_equal", _uniform(6), 4, {0: 1}, 0),                             # a tie with the threshold does not enter
    ("few_positive", _few_positive(), 8, {0: 1}, 0),                      # fewer than k with p > 0; zeros match the mask
    ("shard_bits", random_state(5, 7), 3, {6: 1, 2: 0}, 3 << 5),          # the amplitudes are shard 3 of L = 5
    ("winners_late", ascending(6), 3, {}, 0),                             # the best of block 0 are not the best
    ("sawtooth", sawtooth(6, 16), 20, {}, 0),
]


# ---- the stand-in engine --------------------------------------------------------------------------------------------------------
class TopNumpyEngine(MarginalsNumpyEngine):
    """MarginalsNumpyEngine with ``top_cond`` by the reference; refuses what the entry point refuses (ValueError)"""

    def top_cond(self, k, fix_mask=0, fix_val=0):
        k = int(k)
        if not 1 <= k <= MAX_K:
            raise ValueError("k = %d, 1..%d supported" % (k, MAX_K))
        if fix_val & ~fix_mask:
            raise ValueError("fix_val has bits outside fix_mask")
        if fix_mask >> self.n_qubits:
            raise ValueError("fix_mask has bits at or above qubit %d" % self.n_qubits)
        owned = sorted(self.sh)
        assert owned == list(range(self.world)), "one process"
        amps = np.concatenate([np.asarray(self.sh[s], dtype=np.complex128) for s in owned])
        self.top_calls = getattr(self, "top_calls", 0) + 1
        return top_reference(amps, k, fix_mask, fix_val)


def factory(n, devices=(0,), rank=None, world_size=None):
    return TopNumpyEngine(n, len(devices))


# ---- the QCMRF-level inputs -----------------------------------------------------------------------------------------------------
# graph -> (cliques, seed of conftest.random_theta, the evidence of the conditioned runs)
MODELS = {
    "chain3": ([[0, 1], [1, 2]], 1984, {1: 1}),
    "triangle": ([[0, 1, 2]], 1985, {0: 1}),
    "k4": ([[0, 1, 2, 3]], 1986, {2: 0}),
    "chain8": ([[i, i + 1] for i in range(7)], 1987, {3: 1}),            # 16 qubits: wide enough for a deferred state
}
MODEL_KS = [1, 5]
MIN_GAP = 1e-8


def gaps_ok(p, k):
    """the condition on a model: among the k + 1 largest of the probabilities p every gap exceeds MIN_GAP (so that an
    engine within 1e-10 of p ranks them as the exact pmf does)"""
    top = np.sort(np.asarray(p, dtype=np.float64))[::-1][:k + 1]
    return bool((top[:-1] - top[1:] > MIN_GAP).all())
