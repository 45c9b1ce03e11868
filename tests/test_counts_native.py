"""qcmrf_amd._counts_native.counts_dict (qcmrf_amd/csrc/counts_native.cpp) against the Python code it stands in for:
``_format_keys(*np.unique(words, return_counts=True), num_clbits, creg_sizes)`` and, with weights, the
``np.unique(return_inverse)`` + ``np.bincount`` merge of the multi-rank path.  The dicts are compared as lists of items:
keys, values, value types and insertion order.  Host only, no GPU."""
import sys

import numpy as np
import pytest

from _sampler_reference import exact_index_order, shuffle_swaps, sorted_uniforms, unshuffle
from qcmrf_amd import backend as bk
from qcmrf_amd.backend import _format_keys

WIDTHS = [1, 2, 7, 8, 9, 33, 34, 63, 64]
LENGTHS = [0, 1, 4096, 70000]


@pytest.fixture(autouse=True)
def _native_built():
    assert bk.native_counts_available(), "qcmrf_amd._counts_native is not built (python -m qcmrf_amd.build)"
    assert bk.use_native_counts(True) is True, "the switch must be on by default where the module imports"
    yield
    bk.use_native_counts(True)


def native(words, weights, num_clbits, cregs):
    return bk._counts_native.counts_dict(words, weights, num_clbits, cregs)


def python_counts(words, num_clbits, cregs):
    return _format_keys(*np.unique(words, return_counts=True), num_clbits, cregs)


def python_merge(av, ac, num_clbits, cregs):
    """the merge of (distinct value, count) pairs of several ranks as backend._run_one wrote it before the native call"""
    uv, inv = np.unique(av, return_inverse=True)
    uc = np.bincount(inv, weights=ac, minlength=uv.size).astype(np.int64) if uv.size != av.size else ac[np.argsort(av, kind="stable")]
    return _format_keys(uv, uc, num_clbits, cregs)


def registers(w):
    """register lists of total width w: none, one, two (14 + 20 at w = 34), five with size-1 registers"""
    out = [None, [("c", w)]]
    if w >= 2:
        a = 14 if w == 34 else w // 3 or 1
        out.append([("a", a), ("b", w - a)])
    if w >= 7:
        out.append([("p", 1), ("q", w - 5), ("r", 1), ("s", 2), ("t", 1)])
    return out


def words_of(w, n, kind, seed=5):
    rs = np.random.default_rng(seed + 1000 * w + n)
    top = (1 << w) - 1
    if kind == "equal":
        return np.full(n, top & 0x5A5A5A5A5A5A5A5A | (1 << (w - 1)), dtype=np.uint64)
    if kind == "distinct":
        if w < 20:                                            # as many distinct words as the width has
            n = min(n, 1 << w)
            return rs.permutation(1 << w)[:n].astype(np.uint64)
        x = np.unique(rs.integers(0, top, size=2 * n + 8, dtype=np.uint64, endpoint=True))
        return rs.permutation(x)[:n]
    if kind == "ties":                                        # a handful of values, the extremes and the top bit among them
        pool = np.array([0, top, 1 << (w - 1), top >> 1, 1, top & 0x123456789ABCDEF], dtype=np.uint64)
        return pool[rs.integers(0, pool.size, size=n)]
    x = rs.integers(0, top, size=n, dtype=np.uint64, endpoint=True)     # "random", with 0 and 2^w - 1 put in
    if n >= 2:
        x[n // 2], x[n // 3] = 0, top
    return x


def cases(lengths=LENGTHS):
    for w in WIDTHS:
        for n in lengths:
            for kind in ("random", "equal", "distinct", "ties"):
                if n == 70000 and kind != "ties" and w not in (9, 34, 64):
                    continue                                  # the long inputs at three widths only; ties at every width
                yield w, n, kind


def mismatches(fn, lengths=LENGTHS):
    """every case of ``cases`` x ``registers`` on which ``fn(words, None, w, cregs)`` is not the Python dict"""
    bad = []
    for w, n, kind in cases(lengths):
        words = words_of(w, n, kind)
        keep = words.copy()
        for cregs in registers(w):
            want = python_counts(words, w, cregs)
            got = fn(words, None, w, cregs)
            if got is None or list(got.items()) != list(want.items()) or any(type(v) is not int for v in got.values()):
                bad.append((w, n, kind, cregs))
        assert np.array_equal(words, keep)                    # the caller's buffer is read, never written
    return bad


def test_equals_python_dict():
    assert mismatches(native) == []


def test_top_bit_at_64_is_unsigned():
    words = np.array([1 << 63, 1, (1 << 64) - 1, 0, 1 << 63], dtype=np.uint64)
    got = native(words, None, 64, None)
    assert list(got.items()) == list(python_counts(words, 64, None).items())
    assert list(got.values()) == [1, 1, 2, 1] and list(got)[0] == "0" * 64 and list(got)[-1] == "1" * 64


def test_empty_and_num_clbits_zero():
    empty = np.zeros(0, dtype=np.uint64)
    assert native(empty, None, 34, None) == {} == python_counts(empty, 34, None)
    assert native(empty, np.zeros(0, dtype=np.int64), 34, [("a", 14), ("b", 20)]) == {}
    zeros = np.zeros(17, dtype=np.uint64)
    for cregs in (None, [], [("c", 0)]):
        assert list(native(zeros, None, 0, cregs).items()) == list(python_counts(zeros, 0, cregs).items()) == [("0", 17)]


@pytest.mark.parametrize("w", WIDTHS)
def test_weighted_equals_the_merge_it_replaces(w):
    rs = np.random.default_rng(w)
    for cregs in registers(w):
        # four ranks' (distinct value, count) pairs, the same values on several of them
        parts = [np.unique(words_of(w, 600, "ties" if w < 20 else kind, seed=r), return_counts=True)
                 for r, kind in enumerate(("random", "ties", "random", "ties"))]
        shared = parts[0][0][:50]
        parts.append((shared, rs.integers(1, 9, size=shared.size)))
        av = np.concatenate([p[0] for p in parts])
        ac = np.concatenate([p[1] for p in parts]).astype(np.int64)
        ac[0] = (1 << 31) + 12345                             # a count no 32-bit integer holds
        want = python_merge(av, ac, w, cregs)
        got = native(av, ac, w, cregs)
        assert list(got.items()) == list(want.items())
        assert all(type(v) is int for v in got.values()) and sum(got.values()) == int(ac.sum())
    # every value distinct: the branch of the old code that permutes the counts instead of summing them
    av = words_of(w, 300, "distinct")
    ac = rs.integers(1, 1 << 40, size=av.size).astype(np.int64)
    assert list(native(av, ac, w, None).items()) == list(python_merge(av, ac, w, None).items())


def test_off_path_inputs_answer_none():
    words = words_of(34, 64, "random")
    ok = (words, None, 34, [("a", 14), ("b", 20)])
    assert native(*ok) is not None
    obj = np.empty(3, dtype=object)
    obj[:] = [1 << 70, 2, 3]
    off = [
        (obj, None, 72, None),                                              # registers past 64 bits: Python ints
        (words, None, 65, None),
        (words, None, -1, None),
        (words, None, 34.0, None),
        (words, None, np.int64(34), None),
        (np.arange(128, dtype=np.uint64)[::2], None, 34, None),             # strided
        (words.reshape(8, 8), None, 34, None),
        (words.astype(np.int64), None, 34, None),
        (words.astype(np.uint32), None, 34, None),
        (words.astype(np.float64), None, 34, None),
        (words.tolist(), None, 34, None),
        (None, None, 34, None),
        (words, np.ones(64, dtype=np.uint64), 34, None),                    # weights of the wrong type
        (words, np.ones(63, dtype=np.int64), 34, None),                     # ... of the wrong length
        (words, np.ones(128, dtype=np.int64)[::2], 34, None),
        (words, [1] * 64, 34, None),
        (words, None, 33, None),                                            # a word wider than its key
        (words, None, 34, [("a", 14), ("b", 19)]),                          # registers that do not add up
        (words, None, 34, [("a", 14), ("b", 21)]),
        (words, None, 34, [("a", 34), ("b", 0)]),
        (words, None, 34, [("a", 14), ("b", -20), ("c", 40)]),
        (words, None, 34, [("a", 14), 20]),
        (words, None, 34, [("a", 14.0), ("b", 20)]),
        (words, None, 34, [("a",), ("b", 20)]),
        (words, None, 34, "ab"),
        (words, None, 34, {"a": 14, "b": 20}),
    ]
    for args in off:
        assert native(*args) is None, args
    assert bk._counts_native.counts_dict() is None and bk._counts_native.counts_dict(words) is None


def test_backend_falls_back_to_python():
    """_counts_of on an input the native function declines is the Python dict, and says so"""
    obj = np.empty(4, dtype=object)
    obj[:] = [1 << 70, 2, 1 << 70, 3]
    got, path = bk._counts_of(obj, None, 72, None)
    assert path == "python" and list(got.items()) == list(python_counts(obj, 72, None).items())
    words = words_of(34, 500, "ties")
    loose = [("a", 10), ("b", 20)]                                           # four classical bits in no register
    got, path = bk._counts_of(words, None, 34, loose)
    assert path == "python" and list(got.items()) == list(python_counts(words, 34, loose).items())
    got, path = bk._counts_of(words, None, 34, [("a", 14), ("b", 20)])
    assert path == "native" and list(got.items()) == list(python_counts(words, 34, [("a", 14), ("b", 20)]).items())


def test_switch():
    words = words_of(34, 300, "ties")
    weights = np.arange(1, 301, dtype=np.int64)
    assert bk.use_native_counts(False) is True
    off = bk._counts_of(words, None, 34, None), bk._counts_of(words, weights, 34, None)
    assert bk.use_native_counts(True) is False
    on = bk._counts_of(words, None, 34, None), bk._counts_of(words, weights, 34, None)
    assert [p for _, p in off] == ["python", "python"] and [p for _, p in on] == ["native", "native"]
    for (a, _), (b, _) in zip(off, on):
        assert list(a.items()) == list(b.items())
    assert list(on[1][0].items()) == list(python_merge(words, weights, 34, None).items())


def test_a_wrong_formatter_fails_these_tests():
    """sensitivity: the comparison above notices a formatter that writes the bits in reverse and one that writes the
    registers first to last"""
    def bits_reversed(words, weights, w, cregs):
        return {" ".join(g[::-1] for g in k.split(" ")): v for k, v in native(words, weights, w, cregs).items()}

    def registers_reversed(words, weights, w, cregs):
        return {" ".join(k.split(" ")[::-1]): v for k, v in native(words, weights, w, cregs).items()}

    bad = mismatches(bits_reversed, (1, 4096))
    assert {w for w, _, _, _ in bad} >= set(WIDTHS[1:]), bad[:5]
    bad = mismatches(registers_reversed, (1, 4096))
    assert bad and all(c is not None and len(c) > 1 for _, _, _, c in bad)
    assert {w for w, _, _, _ in bad} >= set(WIDTHS[2:]), bad[:5]


def test_allocated_blocks_do_not_grow():
    words = words_of(34, 48, "ties")
    weights = np.arange(48, dtype=np.int64)
    cregs = [("a", 14), ("b", 20)]
    strided = np.arange(96, dtype=np.uint64)[::2]

    def round_of(n):
        for _ in range(n):
            native(words, None, 34, cregs)
            native(words, weights, 34, None)
            native(strided, None, 34, None)
            native(words, None, 34, [("a", 14), 20])
            native(words, weights[:5], 34, None)
    round_of(200)
    before = sys.getallocatedblocks()
    round_of(4000)                                            # 20 000 calls
    after = sys.getallocatedblocks()
    assert after - before < 50, (before, after)


def test_model_of_the_unshuffled_draw():
    """what qsv_sample_unordered leaves out, at the numpy level: the shuffle permutes the words the walk located and draws
    its random numbers after the spacings, so the words before it are the words after it as a multiset -- and the counts"""
    rs = np.random.default_rng(3)
    p = rs.random(1 << 10) * (rs.random(1 << 10) < 0.3)
    for shots, seed in ((1, 5), (2, 6), (4096, 7)):
        total = float(p.sum())
        r = sorted_uniforms(seed, shots, total)
        unshuffled = exact_index_order(p, r)[0]
        shuffled = unshuffled.tolist()
        for s, k in zip(*(a.tolist() for a in shuffle_swaps(seed, shots))):
            shuffled[s], shuffled[k] = shuffled[k], shuffled[s]
        shuffled = np.array(shuffled, dtype=np.uint64)
        assert np.array_equal(unshuffle(seed, shots, shuffled), unshuffled)
        assert np.array_equal(np.sort(shuffled), np.sort(unshuffled))
        assert shots < 64 or not np.array_equal(shuffled, unshuffled)
        assert list(native(shuffled, None, 10, None).items()) == list(native(unshuffled, None, 10, None).items()) \
            == list(python_counts(shuffled, 10, None).items())
