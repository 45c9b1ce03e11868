"""Implied zeros (option implied_zeros): the generator as a program's last pass leaves the provably-zero
part of a shard unwritten and says so in the shard's zmask.  Every reader must give exactly what the
full write (implied_zeros = 0) gives -- counts, amplitudes, norm, marginals, expectation values -- and
must never see the undefined memory, which these tests fill with NaN first."""
import numpy as np
import pytest

from conftest import random_theta
from oracle import closed_form as cf, gate_stream as gs

pytestmark = pytest.mark.gpu

NAN = complex(float("nan"), float("nan"))


@pytest.fixture(scope="module")
def be():
    from qcmrf_amd.backend import QsvBackend
    b = QsvBackend()
    yield b
    b.close()


def _same(a, b):
    """equal element by element (a zero's sign may differ) and free of NaN; tuples element by element"""
    if isinstance(a, tuple):
        return isinstance(b, tuple) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    if np.issubdtype(a.dtype, np.inexact) and np.isnan(a).any():
        return False
    return a.shape == b.shape and bool((a == b).all())


def _close(a, b):
    """marginals: k_marginal adds with atomics, so the order of the additions (and the last bit) may vary"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and not np.isnan(a).any() and np.allclose(a, b, rtol=1e-13, atol=0.0)


def _observe(be, qc, n, **opts):
    """everything a caller reads after one run, in a fixed order"""
    counts = be.run(qc, shots=3000, seed_simulator=7, **opts).result().get_counts()
    eng, pl = be.last_engine, be.last_plan
    kinds = eng.stats()["kinds"]
    amp = be.statevector()
    norm = eng.norm()
    rs = np.random.RandomState(3)
    diag = rs.randn(2 ** 4)
    ex_post = be.expectation_diagonal(diag, [0, 1, 2, 3], fixed={j: 0 for j in range(n, qc.num_qubits)})
    ex_all = be.expectation_diagonal(diag, [0, 1, 2, 3])
    prob = eng.probabilities([pl.layout[q] for q in (0, 1, n - 1, qc.num_qubits - 1)])
    return dict(counts=counts, kinds=kinds, amp=amp, norm=norm, ex_post=ex_post, ex_all=ex_all, prob=prob)


@pytest.mark.parametrize("n,devices,layout", [
    (8, 1, "auto"), (8, 2, "auto"), (8, 4, "auto"), (8, 1, "reference"),
    (12, 1, "reference"), (12, 4, "auto"), (14, 1, "auto"), (14, 2, "reference"),
])
def test_same_result_as_full_write(be, n, devices, layout):
    """QCMRF chains of W = 2n = 16..28 qubits, fold_fresh on: implied_zeros 1 against 0 at the same seed.
    The AND scratch qubit lands on a register bit (auto layout below 33 local qubits: bit 10; reference at n = 8),
    a thread bit (reference, n = 12) or a block bit (reference, n = 14)."""
    from qcmrf_amd import QCMRF
    C = gs.chain_cliques(n)
    th = random_theta(cf.model_shape(C)[3], seed=n + devices)
    qc = QCMRF(C, th)
    got = {}
    for iz in (1, 0):
        got[iz] = _observe(be, qc, n, devices=(0,) * devices, layout=layout, engine_options={"implied_zeros": iz})
    a, b = got[1], got[0]
    assert a["counts"] == b["counts"]
    assert _same(a["amp"], b["amp"])
    assert np.abs(a["amp"] - cf.amplitudes(C, th)).max() < 1e-12
    assert a["norm"] == b["norm"] and a["ex_post"] == b["ex_post"] and a["ex_all"] == b["ex_all"]
    assert _close(a["prob"], b["prob"])
    # the generator wrote half the shard and nothing filled the other half during the run
    L = qc.num_qubits - (devices.bit_length() - 1)
    assert a["kinds"]["init_prod"]["bytes"] == devices * 16.0 * 2 ** (L - 1), a["kinds"]
    assert b["kinds"]["init_prod"]["bytes"] == devices * 16.0 * 2 ** L, b["kinds"]
    assert "init" not in a["kinds"] and "init" not in b["kinds"]
    be.run(QCMRF([[0, 1]], [-0.1] * 4), shots=1)


def _program(W, zero_qubits, seed):
    from qcmrf_amd import ir, program
    rs = np.random.RandomState(seed)
    mask = (1 << W) - 1
    for q in zero_qubits:
        mask &= ~(1 << q)
    ops = [ir.op_init(mask)]
    for _ in range(10):
        k = int(rs.randint(1, 5))
        qs = [int(q) for q in rs.choice([q for q in range(W) if q not in zero_qubits], size=k, replace=False)]
        ops.append(ir.op_diag(qs, np.exp(1j * rs.randn(2 ** k)) * (0.5 + rs.rand(2 ** k))))
    return program.encode(ops)


def _poisoned(W, devices, opts):
    from qcmrf_amd import _lib
    eng = _lib.Engine(W, devices=devices)
    for k, v in opts.items():
        eng.set_option(k, v)
    eng.set_amplitudes(0, np.full(2 ** W, NAN))
    return eng


def _unitary(k, seed):
    rs = np.random.RandomState(seed)
    q, r = np.linalg.qr(rs.randn(2 ** k, 2 ** k) + 1j * rs.randn(2 ** k, 2 ** k))
    return q * (np.diag(r) / np.abs(np.diag(r)))


READERS = ["sample", "norm", "expect", "expect_post", "prob", "amp", "blocksum", "copy", "copy_exec", "exec_no_init",
           "apply_1q", "apply_kq", "swap_local", "swap_shard", "set_partial"]


@pytest.mark.parametrize("zq,devices,bit0", [
    (15, 1, 0),        # top bit: a block bit of the bits-6.. tile
    (15, 1, -1),       # top bit on a register bit (the tile on the top bits, as at 34 qubits)
    (8, 1, 0),         # a register bit of the bits-6.. tile
    (2, 1, 0),         # a thread bit
    (12, 2, 0),        # two virtual shards: the top local bit is a wave bit
    (13, 4, 0),        # four: a block bit of every shard
])
def test_poisoned_memory_never_read(zq, devices, bit0):
    """NaN everywhere, then the generator program, then ONE reader -- every reader gets a state of its own whose zero
    half is still implied (checked through the bytes the generator was charged).  Each must match implied_zeros = 0
    without a NaN, and the numpy engine where it changes the state: sample, norm, expect_diag (plain and post-selected),
    probabilities, amplitudes, norm + sample without tile sums (block-sum pass), copy_state then amplitudes, copy_state
    then a qsv_exec without an init, such an exec on the state itself, a one-qubit gate on the zero qubit, a dense
    4-qubit gate on it, a local swap of it, its exchange with a shard bit (virtual shards), a partial write into the
    zero half."""
    from qcmrf_amd import _lib, ir, program
    from oracle.sharded_numpy import NumpyEngine
    W = 16
    devs = (0,) * devices
    L = W - (devices.bit_length() - 1)
    rec, data = _program(W, [zq], seed=zq)
    h = np.array([[1, 1], [1, -1]], dtype=np.complex128) / np.sqrt(2.0)
    after_rec, after_data = program.encode([ir.op_diag([zq, 3], np.exp(1j * np.arange(4.0))), ir.op_u(zq, h), ir.op_u(5, h)])
    u4 = _unitary(4, zq)
    kq_qubits = [3, zq, 9, 1] if zq not in (3, 9, 1) else [4, zq, 10, 0]
    table = np.random.RandomState(1).randn(2 ** 4)
    vals = np.arange(1, 9) * (1 + 1j)

    def ref_state(name):
        ref = NumpyEngine(W)
        ref.exec(rec, data)
        if name in ("copy_exec", "exec_no_init"):
            ref.exec(after_rec, after_data)
        elif name == "apply_1q":
            ref.apply_1q(zq, h)
        elif name == "apply_kq":
            ref.apply_kq(kq_qubits, u4)
        elif name == "swap_local":
            ref.swap_layout([zq], [4])
        elif name == "swap_shard":
            ref.swap_layout([zq], [W - 1])
        amp = ref.amplitudes()
        if name == "set_partial":
            amp[(1 << zq) + 100: (1 << zq) + 108] = vals
        return amp

    def read(eng, other, name):
        if name == "sample":
            return eng.sample(2000, 5)
        if name == "norm":
            return eng.norm()
        if name == "expect":
            return eng.expect_diag([zq, 0, 7, 14], table)
        if name == "expect_post":
            return eng.expect_diag([1, 2, 9, 11], table, fix_mask=1 << zq, fix_val=0)
        if name == "prob":
            return eng.probabilities([zq, 0, 10, 15])
        if name == "blocksum":
            return eng.norm(), eng.sample(2000, 5)
        if name in ("copy", "copy_exec"):
            other.copy_from(eng)
            if name == "copy_exec":
                other.exec(after_rec, after_data)
            return other.amplitudes()
        if name == "exec_no_init":
            eng.exec(after_rec, after_data)
        elif name == "apply_1q":
            eng.apply_1q(zq, h)
        elif name == "apply_kq":
            eng.apply_kq(kq_qubits, u4)
        elif name == "swap_local":
            eng.swap_layout([zq], [4])
        elif name == "swap_shard":
            eng.swap_layout([zq], [W - 1])
        elif name == "set_partial":
            eng.set_amplitudes((1 << zq) + 100, vals)
        return eng.amplitudes()

    readers = [r for r in READERS if r != "swap_shard" or devices > 1]
    res = {}
    for iz in (1, 0):
        eng = _lib.Engine(W, devices=devs)
        other = _lib.Engine(W, devices=devs)
        eng.set_option("implied_zeros", iz)
        eng.set_option("init_prod_bit0", bit0)
        for name in readers:
            for e in (eng, other):
                e.set_amplitudes(0, np.full(2 ** W, NAN))
            eng.set_option("fused_sums", 0 if name == "blocksum" else 1)
            eng.reset_stats()
            eng.exec(rec, data)
            kinds = eng.stats()["kinds"]
            # the reader below sees the zero half implied (iz = 1): only half the shard was written, nothing filled it
            assert set(kinds) == {"init_prod"}, (name, kinds)
            assert kinds["init_prod"]["bytes"] == devices * 16.0 * 2 ** (L - (1 if iz else 0)), (name, kinds)
            res[iz, name] = read(eng, other, name)
        eng.close()
        other.close()
    for name in readers:
        a, b = res[1, name], res[0, name]
        if name == "prob":
            assert _close(a, b), name
        else:
            assert _same(a, b), name
        if isinstance(a, np.ndarray) and a.dtype == np.complex128:
            assert np.abs(a - ref_state(name)).max() < 1e-12, name


def test_failed_program_keeps_implied_zeros():
    """a program whose init is parsed but never written (a later op is rejected) leaves the previous state readable:
    the shard's zmask still describes the memory"""
    from qcmrf_amd import _lib, ir, program
    W, zq = 16, 15
    rec, data = _program(W, [zq], seed=3)
    bad_rec, bad_data = program.encode([ir.op_init((1 << W) - 1), ir.op_diag([0, 1], np.ones(4))])
    bad_rec[1]["data_off"] = 1 << 40                      # outside the data pool: qsv_exec fails at this op
    with _lib.Engine(W) as eng:
        eng.set_amplitudes(0, np.full(2 ** W, NAN))
        eng.exec(rec, data)
        want = eng.amplitudes()
        assert not np.isnan(want).any()
        with pytest.raises(Exception):
            eng.exec(bad_rec, bad_data)
        assert _same(eng.amplitudes(), want)
        assert abs(eng.norm() - (np.abs(want) ** 2).sum()) < 1e-12


def test_partial_write_into_zero_region_kept():
    """qsv_set_amplitudes into the implied-zero half: the rest of that half reads back as zeros, the written
    values as written"""
    from qcmrf_amd import _lib
    W, zq = 16, 15
    rec, data = _program(W, [zq], seed=2)
    with _lib.Engine(W) as eng:
        eng.set_amplitudes(0, np.full(2 ** W, NAN))
        eng.exec(rec, data)
        want = eng.amplitudes()
        assert not np.isnan(want).any() and (want[2 ** zq:] == 0).all()
        vals = np.arange(1, 9) * (1 + 1j)
        eng.set_amplitudes(2 ** zq + 100, vals)
        want[2 ** zq + 100: 2 ** zq + 108] = vals
        assert _same(eng.amplitudes(), want)
        assert abs(eng.norm() - (np.abs(want) ** 2).sum()) < 1e-12


def test_zero_tracking_leaves_no_fill(be):
    """the opt-in zero-tracking path ends without its trailing fill: implied zeros, same counts and amplitudes"""
    from qcmrf_amd import QCMRF
    C = gs.chain_cliques(8)
    th = random_theta(cf.model_shape(C)[3], seed=4)
    got = {}
    for iz in (1, 0):
        got[iz] = _observe(be, QCMRF(C, th), 8, fold_fresh=False, engine_options={"implied_zeros": iz, "zero_tracking": 1})
    assert got[1]["counts"] == got[0]["counts"] and _same(got[1]["amp"], got[0]["amp"])
    assert "init" not in got[1]["kinds"]
    assert got[1]["norm"] == got[0]["norm"] and got[1]["ex_post"] == got[0]["ex_post"]
    be.run(QCMRF([[0, 1]], [-0.1] * 4), shots=1)
