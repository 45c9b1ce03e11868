"""Programs and runners shared by tests/test_gpu_deferred_state.py: an init followed by diagonal factors only (the
generator is the program's only pass), run once with defer_state=0 -- the writing generator, pinned to numpy and the
closed form by test_gpu_generator*.py -- and once with defer_state=1 on a second engine of the same build.

W = 16, R = 4 on the top bits (init_prod_bit0 -1): lane bits 0..4 and 11, wave bits 5 and 6, block bits 7..10 (the
tile index), register bits 12..15."""
import numpy as np

W = 16
REG_BIT, THREAD_BIT, BLOCK_BIT = 15, 3, 9
BLOCK = [7, 8, 9, 10]
SHOTS = 3000
SEED = 11


def table(rs, k):
    return np.exp(1j * rs.randn(2 ** k)) * (0.5 + rs.rand(2 ** k))


def random_factors(w, zero, n, seed, kmax=4):
    rs = np.random.RandomState(seed)
    pool = [q for q in range(w) if q not in zero]
    out = []
    for _ in range(n):
        k = int(rs.randint(1, min(kmax, len(pool)) + 1))
        out.append([int(q) for q in rs.choice(pool, size=k, replace=False)])
    return out


def program_ops(w, zero, factors, seed, tables=None):
    """init (every qubit but ``zero`` uniform) and one diagonal per factor; tables: {factor number: table} overrides"""
    from qcmrf_amd import ir
    rs = np.random.RandomState(seed)
    mask = (1 << w) - 1
    for q in zero:
        mask &= ~(1 << q)
    ops = [ir.op_init(mask)]
    for i, qs in enumerate(factors):
        t = table(rs, len(qs))
        if tables and i in tables:
            t = np.asarray(tables[i], dtype=np.complex128)
        ops.append(ir.op_diag(qs, t))
    return ops


def default_ops(seed=1, zero=(REG_BIT,), n=14, w=W):
    return program_ops(w, list(zero), random_factors(w, list(zero), n, seed=seed), seed=seed + 100)


def start(ops, defer, w=W, devices=1, **opts):
    """a fresh engine with the program run on it; the caller closes it"""
    from qcmrf_amd import _lib, program
    rec, data = program.encode(ops)
    eng = _lib.Engine(w, devices=(0,) * devices)
    for k, v in opts.items():
        eng.set_option(k, v)
    eng.set_option("defer_state", defer)
    eng.reset_stats()
    eng.exec(rec, data)
    return eng


def init_prod_bytes(eng):
    k = eng.stats()["kinds"].get("init_prod")
    assert k is not None and k["launches"] >= 1, eng.stats()
    return k["bytes"]


def check_pair(ops, w=W, devices=1, shots=SHOTS, **opts):
    """The program on the writing path and deferred.  Deferred: nothing stored (0 bytes booked), the same words for
    the same seed, still deferred after a second sample with another seed, and then -- realised once per shard -- the
    same amplitudes bit for bit and the bytes the writing path books."""
    e0 = start(ops, 0, w, devices, **opts)
    e1 = start(ops, 1, w, devices, **opts)
    try:
        i0 = e0.state_info()
        assert not i0["deferred"] and i0["listed_launches"] == 0
        want_bytes = init_prod_bytes(e0)
        assert want_bytes > 0
        i1 = e1.state_info()
        assert i1["deferred"] and i1["realize_calls"] == 0, i1
        assert init_prod_bytes(e1) == 0.0
        assert e1.norm() == e0.norm()
        w0, w1 = e0.sample(shots, SEED), e1.sample(shots, SEED)
        assert np.array_equal(w0, w1)
        i1 = e1.state_info()
        assert i1["deferred"] and i1["realize_calls"] == 0 and i1["listed_launches"] >= 1, i1
        assert np.array_equal(e0.sample(shots, SEED + 1), e1.sample(shots, SEED + 1))
        i1 = e1.state_info()
        assert i1["deferred"] and i1["realize_calls"] == 0, i1
        assert init_prod_bytes(e1) == 0.0
        a0, a1 = e0.amplitudes(), e1.amplitudes()
        assert np.array_equal(a0.view(np.uint64), a1.view(np.uint64))
        i1 = e1.state_info()
        assert not i1["deferred"] and i1["realize_calls"] == devices, i1
        assert init_prod_bytes(e1) == want_bytes
        assert e0.state_info()["realize_calls"] == 0
        return a0, w0
    finally:
        e0.close()
        e1.close()


def check_reader(read, ops=None, w=W, opts=None, before=None, compare=None):
    """``read(engine)`` after the program on both paths: equal results bit for bit, the deferred shard realised exactly
    once, and the init_prod bytes the writing path books.  before(engine) runs on both engines right after the program.
    compare(r0, r1, amplitudes): for a reader whose own result is not reproducible to the bit from call to call (sums
    by floating-point atomics); the state it read is compared bit for bit all the same."""
    ops = default_ops() if ops is None else ops
    e0 = start(ops, 0, w, **(opts or {}))
    e1 = start(ops, 1, w, **(opts or {}))
    try:
        assert e1.state_info()["deferred"]
        if before is not None:
            before(e0)
            before(e1)
        r0, r1 = read(e0), read(e1)
        i1 = e1.state_info()
        assert not i1["deferred"] and i1["realize_calls"] == 1, i1
        assert e0.state_info()["realize_calls"] == 0
        assert init_prod_bytes(e1) == init_prod_bytes(e0)
        # the state itself, whatever the reader returned
        amp = e0.amplitudes()
        same(amp, e1.amplitudes())
        if compare is None:
            same(r0, r1)
        else:
            compare(r0, r1, amp)
        assert e1.state_info()["realize_calls"] == 1
    finally:
        e0.close()
        e1.close()


def same(a, b):
    if isinstance(a, (tuple, list)):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            same(x, y)
        return
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype
    assert a.tobytes() == b.tobytes()
