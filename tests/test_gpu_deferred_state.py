"""Deferred state (option defer_state): the generator as a program's last pass leaves tile sums and stores nothing; the
sampler stores the tiles its shots fall into (the generator's listed form); every other reader has the state written
first (realize).  Every case forces defer_state=1 at 16-18 qubits and is compared, bit for bit, against defer_state=0 of
the same build: the writing generator, which test_gpu_generator*.py pin to numpy and the closed form."""
import numpy as np
import pytest

from _deferred_cases import (BLOCK, BLOCK_BIT, REG_BIT, THREAD_BIT, W, check_pair, check_reader, default_ops,
                             init_prod_bytes, program_ops, random_factors, same, start)

pytestmark = pytest.mark.gpu


# ---- counts equality: the same words for the same seed, then the same amplitudes -------------------------------------
@pytest.mark.parametrize("bit0", [0, -1, 6])
@pytest.mark.parametrize("r", [3, 4, 5, 6])
def test_tile_shapes(r, bit0):
    check_pair(default_ops(seed=r), init_prod_r=r, init_prod_bit0=bit0)


@pytest.mark.parametrize("group", [0, 1, 2, 3])
def test_group_bits(group):
    check_pair(default_ops(seed=20 + group), init_prod_r=4, init_prod_bit0=-1, init_prod_group=group)


@pytest.mark.parametrize("zq", [REG_BIT, THREAD_BIT, BLOCK_BIT])
@pytest.mark.parametrize("iz", [0, 1])
def test_implied_zeros(iz, zq):
    """the zero qubit on a register, a thread and a block bit; implied zeros on and off"""
    check_pair(default_ops(seed=30 + zq, zero=(zq,)), init_prod_r=4, init_prod_bit0=-1, implied_zeros=iz)


@pytest.mark.parametrize("nt", [0, 1])
def test_nontemporal(nt):
    check_pair(default_ops(seed=40), init_prod_nt=nt)


@pytest.mark.parametrize("grid", [1, 3])
def test_grid(grid):
    check_pair(default_ops(seed=50 + grid), init_prod_r=4, init_prod_bit0=-1, init_prod_grid=grid)


@pytest.mark.parametrize("devices", [1, 2, 4])
def test_virtual_shards(devices):
    check_pair(default_ops(seed=60 + devices), devices=devices)


def test_more_than_64_factors():
    """100 factors in one generator pass: factors 64.. on the second descriptor lane"""
    ops = program_ops(W, [REG_BIT], random_factors(W, [REG_BIT], 100, seed=2, kmax=3), seed=4)
    check_pair(ops, init_prod_r=4, init_prod_bit0=-1, pass_max_ops=512)


def test_more_shots_than_the_grid():
    check_pair(default_ops(seed=70), shots=70000)


def test_most_shots_in_one_tile():
    """every block bit weighted 1 : 1e-3 towards 0: most shots share tile 0, so the list is mostly duplicates"""
    fl = [[q] for q in BLOCK] + random_factors(W, [REG_BIT] + BLOCK, 8, seed=5)
    ops = program_ops(W, [REG_BIT], fl, seed=6, tables={i: [1.0, 1e-3] for i in range(len(BLOCK))})
    _, words = check_pair(ops, init_prod_r=4, init_prod_bit0=-1)
    block_mask = sum(1 << q for q in BLOCK)
    assert int(((words & np.uint64(block_mask)) == 0).sum()) > len(words) * 0.9


def test_tiles_with_sum_zero():
    """a factor that is 0 where block bit 8 is 1: half of the tiles have sum 0 (and are stored nowhere in the list)"""
    fl = [[8]] + random_factors(W, [REG_BIT], 10, seed=7)
    ops = program_ops(W, [REG_BIT], fl, seed=8, tables={0: [1.0, 0.0]})
    amp, words = check_pair(ops, init_prod_r=4, init_prod_bit0=-1)
    assert not (words & np.uint64(1 << 8)).any()
    assert (np.abs(amp[words.astype(np.int64)]) > 0).all()


# ---- readers: realised exactly once, results and state bit for bit ---------------------------------------------------
H = np.array([[1, 1], [1, -1]], dtype=np.complex128) / np.sqrt(2.0)


def _second_program(eng):
    from qcmrf_amd import ir, program
    rec, data = program.encode([ir.op_diag([2, 13], np.exp(1j * np.arange(4))), ir.op_u(5, H)])
    eng.exec(rec, data)
    return eng.amplitudes()


def _copy(eng):
    from qcmrf_amd import _lib
    other = _lib.Engine(W)
    try:
        other.copy_from(eng)
        assert not other.state_info()["deferred"]
        return other.amplitudes()
    finally:
        other.close()


def _set_some(eng):
    eng.set_amplitudes(100, np.array([0.125 + 0.25j, -0.5j, 0.75]))
    return eng.amplitudes(96, 16)


def _gate(eng):
    eng.apply_1q(5, H)
    return eng.amplitudes()


def _swap(eng):
    eng.swap_layout([2], [13])
    return eng.amplitudes()


READERS = {
    "amplitudes": lambda e: e.amplitudes(),
    "amplitudes_slice": lambda e: e.amplitudes(12345, 777),
    "expectation_diagonal": lambda e: np.array(e.expect_diag([1, 8, 12], np.arange(8.0) - 3.0, fix_mask=1 << 4, fix_val=0)),
    "gate_then_amplitudes": _gate,
    "exec_without_init": _second_program,
    "copy_state": _copy,
    "partial_set_amplitudes": _set_some,
    "layout_swap": _swap,
}


@pytest.mark.parametrize("name", sorted(READERS))
def test_reader(name):
    check_reader(READERS[name])


def test_reader_probabilities():
    """k_marginal adds |a|^2 into its bins with floating-point atomics, in whatever order the hardware takes them: two
    calls on one and the same state differ in the last bits, so bit equality of the marginal is not a property either
    path has.  The state the reader saw is compared bit for bit (check_reader); each marginal is held to the exact one
    of those amplitudes (math.fsum) within the reordering bound of a sum of N = 2^16 / 16 non-negative terms,
    (N - 1) * 2^-53 relative (Higham, recursive summation in any order), here doubled for the |a|^2 roundings."""
    import math
    qubits = [0, 3, 9, 14]

    def compare(r0, r1, amp):
        p = amp.real ** 2 + amp.imag ** 2
        idx = np.arange(amp.size)
        j = sum(((idx >> q) & 1) << b for b, q in enumerate(qubits))
        exact = np.array([math.fsum(p[j == k]) for k in range(1 << len(qubits))])
        bound = 2.0 * (amp.size / 16 - 1) * 2.0 ** -53 * exact
        for r in (r0, r1):
            err = np.abs(r - exact)
            print("probabilities: max err / bound", float((err / bound).max()))
            assert (err <= bound).all()

    check_reader(lambda e: e.probabilities(qubits), compare=compare)


def test_reader_norm_without_cached_sums():
    """cache_sums=0: qsv_norm runs the block-sum pass over the amplitudes"""
    check_reader(lambda e: np.float64(e.norm()), before=lambda e: e.set_option("cache_sums", 0))


def test_reader_sample_block_sum_fallback():
    """qsv_sample off the tile path (block sums and k_locate over the amplitudes): the state is realised first.  The
    fallback is reached with cache_sums=0 after the program; fused_sums=0 before the program leaves no tile sums, so
    defer_state is ignored there (test_ignored_without_tile_sums)."""
    check_reader(lambda e: e.sample(2000, 5), before=lambda e: e.set_option("cache_sums", 0))


def test_ignored_without_tile_sums():
    """fused_sums=0: the generator leaves no tile sums, defer_state=1 is ignored, sample takes the fallback"""
    ops = default_ops(seed=3)
    e0, e1 = start(ops, 0, fused_sums=0), start(ops, 1, fused_sums=0)
    try:
        assert not e1.state_info()["deferred"]
        assert init_prod_bytes(e1) == init_prod_bytes(e0) > 0
        same(e0.sample(2000, 5), e1.sample(2000, 5))
        same(e0.amplitudes(), e1.amplitudes())
        assert e1.state_info() == {"deferred": False, "realize_calls": 0, "listed_launches": 0}
    finally:
        e0.close()
        e1.close()


def test_ignored_when_not_the_last_pass():
    """a gate after the factors: the generator is not the program's final pass and writes"""
    from qcmrf_amd import ir
    ops = default_ops(seed=4) + [ir.op_u(5, H)]
    e0, e1 = start(ops, 0), start(ops, 1)
    try:
        assert not e1.state_info()["deferred"]
        same(e0.sample(2000, 5), e1.sample(2000, 5))
        same(e0.amplitudes(), e1.amplitudes())
        assert e1.state_info()["realize_calls"] == 0
    finally:
        e0.close()
        e1.close()


# ---- stale memory, failure path --------------------------------------------------------------------------------------
def test_stale_memory():
    """program A written, then program B deferred on the same engine: B's counts, then B's amplitudes (a reader that
    did not realise would return A's)"""
    from qcmrf_amd import program
    a, b = default_ops(seed=8), default_ops(seed=9)
    ref = start(b, 0)
    eng = start(a, 0)
    try:
        amp_a = eng.amplitudes()
        eng.set_option("defer_state", 1)
        eng.exec(*program.encode(b))
        assert eng.state_info()["deferred"]
        same(ref.sample(3000, 2), eng.sample(3000, 2))
        assert eng.state_info()["deferred"]
        amp_b = eng.amplitudes()
        same(ref.amplitudes(), amp_b)
        assert not np.array_equal(amp_a, amp_b)
        assert eng.state_info()["realize_calls"] == 1
    finally:
        ref.close()
        eng.close()


def test_refused_program_keeps_the_deferred_state():
    """a program refused at a later op, before its init writes: the deferred state and its recipe stand"""
    from qcmrf_amd import program
    ops = default_ops(seed=10)
    ref = start(ops, 0)
    eng = start(ops, 1)
    try:
        rec, data = program.encode(default_ops(seed=11, zero=(THREAD_BIT,)))
        rec = rec.copy()
        rec[-1]["qubits"][0] = W + 3                      # no such qubit: refused when that op is parsed
        with pytest.raises(ValueError):
            eng.exec(rec, data)
        assert eng.state_info() == {"deferred": True, "realize_calls": 0, "listed_launches": 0}
        same(ref.sample(3000, 2), eng.sample(3000, 2))
        same(ref.amplitudes(), eng.amplitudes())
        assert eng.state_info()["realize_calls"] == 1
    finally:
        ref.close()
        eng.close()


def test_next_init_ends_deferral_without_realising():
    from qcmrf_amd import program
    a, b = default_ops(seed=12), default_ops(seed=13)
    ref = start(b, 0)
    eng = start(a, 1)
    try:
        eng.set_option("defer_state", 0)
        eng.exec(*program.encode(b))
        assert eng.state_info() == {"deferred": False, "realize_calls": 0, "listed_launches": 0}
        same(ref.amplitudes(), eng.amplitudes())
    finally:
        ref.close()
        eng.close()


# ---- backend ---------------------------------------------------------------------------------------------------------
def _chain():
    from oracle import gate_stream as gs
    from qcmrf_amd import QCMRF
    return QCMRF(gs.chain_cliques(9), (-np.linspace(0.05, 1.5, 32)).tolist())     # 18 qubits: the generator runs


def test_backend_auto_gate_and_forced():
    """defer_state unset at 18 qubits: nothing deferred (auto starts at 30 local qubits).  Forced: deferred through
    run() and get_counts(), realised once by statevector(), the same counts and amplitudes."""
    from qcmrf_amd import Aer
    backend = Aer.get_backend("qasm_simulator")
    try:
        qc = _chain()
        c0 = backend.run(qc, shots=2048, seed_simulator=7).result().get_counts()
        info = backend.last_engine.state_info()
        assert info == {"deferred": False, "realize_calls": 0, "listed_launches": 0}
        sv0 = backend.statevector()
        assert backend.last_engine.state_info()["realize_calls"] == 0
        c1 = backend.run(qc, shots=2048, seed_simulator=7, engine_options={"defer_state": 1}).result().get_counts()
        info = backend.last_engine.state_info()
        assert info["deferred"] and info["realize_calls"] == 0 and info["listed_launches"] == 1, info
        assert c1 == c0
        sv1 = backend.statevector()
        info = backend.last_engine.state_info()
        assert not info["deferred"] and info["realize_calls"] == 1
        same(sv0, sv1)
        # the option was this run's: the next one is back on the auto gate
        backend.run(qc, shots=16, seed_simulator=7).result()
        assert not backend.last_engine.state_info()["deferred"]
    finally:
        backend.close()


def test_backend_never_defers_without_shots():
    from qcmrf_amd import Aer
    backend = Aer.get_backend("qasm_simulator")
    try:
        qc = _chain()
        backend.run(qc, shots=0, seed_simulator=7).result()
        assert not backend.last_engine.state_info()["deferred"]
        # an engine that would defer whenever it may: run(shots=0) still turns it off, unless the caller asks
        backend.last_engine.set_option("defer_state", 1)
        backend.run(qc, shots=0, seed_simulator=7).result()
        assert not backend.last_engine.state_info()["deferred"]
        backend.run(qc, shots=0, seed_simulator=7, engine_options={"defer_state": 1}).result()
        assert backend.last_engine.state_info()["deferred"]
    finally:
        backend.close()
