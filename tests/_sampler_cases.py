"""The states and calls of the exact sampler tests (test infrastructure): seeded numpy states, so that the host suite
can show that no uniform of any call lands within the tolerance of a prefix boundary (test_sampler_reference.py) and
the GPU suite can then demand every word (test_gpu_sampler_exact.py).

INDEX_CASES: name -> (n qubits, P virtual shards, [(state, [(shots, seed), ...]), ...]); the states of one case are
loaded one after another into ONE engine and sampled with the calls listed."""
import numpy as np

BLOCK = 4096          # QSV_SBLOCK: amplitudes per sampling block
ROW = 64              # one wavefront row of k_locate


def rand_state(n, seed):
    rs = np.random.RandomState(seed)
    v = rs.randn(2 ** n) + 1j * rs.randn(2 ** n)
    return v / np.linalg.norm(v)


def probs(v):
    """|amp|^2 the way every test here forms it (re^2 + im^2 in float64)"""
    v = np.asarray(v, dtype=np.complex128)
    return v.real * v.real + v.imag * v.imag


def _normed(v):
    return v / np.linalg.norm(v)


def half_empty(n=10, seed=29):
    """the state of test_sampling_matches_distribution: bit 3 structurally |0>"""
    v = rand_state(n, seed)
    v[(np.arange(2 ** n) & 0b1000) != 0] = 0
    return _normed(v)


def first_block_zero():
    v = rand_state(13, 31)
    v[:BLOCK] = 0
    return _normed(v)


def last_block_zero():
    v = rand_state(13, 32)
    v[BLOCK:] = 0
    return _normed(v)


def rows_zero():
    """whole 64-amplitude rows empty inside both blocks: every third row, the rows on either side of the block seam,
    the first row of the state and the last one"""
    v = rand_state(13, 33).reshape(-1, ROW)
    rows = np.arange(v.shape[0])
    v[(rows % 3 == 1) | np.isin(rows, [0, 63, 64, 127])] = 0
    return _normed(v.ravel())


def shards_1_3_empty():
    v = rand_state(14, 37)
    v[BLOCK:2 * BLOCK] = 0
    v[3 * BLOCK:] = 0
    return _normed(v)


def heavy_shard():
    """shard 0 of 2 carries 97 % of the mass"""
    v = rand_state(16, 41)
    h = v.size // 2
    m0, m1 = np.linalg.norm(v[:h]) ** 2, np.linalg.norm(v[h:]) ** 2
    v[h:] *= np.sqrt(0.03 / 0.97 * m0 / m1)
    return _normed(v)


def one_index():
    v = np.zeros(2 ** 12, dtype=np.complex128)
    v[1234] = 1.0
    return v


def last_amp_plus_tiny():
    """all mass on the last amplitude of the last block, 2^-40 of it on index 0"""
    v = np.zeros(2 ** 12, dtype=np.complex128)
    v[-1] = 1.0
    v[0] = 2.0 ** -20
    return v


def unnormalised():
    return rand_state(13, 43) * np.sqrt(3.7)


INVALIDATION_U = np.array([[0.6, 0.8j], [0.8j, 0.6]])          # unitary, mixes |0> and |1> of its target unevenly
INVALIDATION_T = 5


def invalidation_states():
    a = rand_state(12, 47)
    b = rand_state(12, 48)
    b[(np.arange(b.size) & 0b100000) != 0] = 0             # qubit 5 structurally |0> before the gate ...
    b = _normed(b)
    c = b.reshape(-1, 2, 2 ** INVALIDATION_T)                # ... and 0.36 / 0.64 after it
    c = np.einsum("ab,ibj->iaj", INVALIDATION_U, c).reshape(-1)
    return a, b, c


def _invalidation_steps():
    a, b, c = invalidation_states()
    return [(a, [(6000, 61)]), (b, [(6000, 62)]), (c, [(6000, 63)])]


INDEX_CASES = {
    "sub_block_half_empty": (10, 1, lambda: [(half_empty(), [(20000, 1234)])]),
    "first_block_zero": (13, 1, lambda: [(first_block_zero(), [(12000, 51)])]),
    "last_block_zero": (13, 1, lambda: [(last_block_zero(), [(12000, 52)])]),
    "rows_zero": (13, 1, lambda: [(rows_zero(), [(12000, 53)])]),
    "shards_1_3_empty": (14, 4, lambda: [(shards_1_3_empty(), [(12000, 54)])]),
    "heavy_shard_buffer_growth": (16, 2, lambda: [(heavy_shard(), [(100, 55), (70000, 56)])]),
    "one_index": (12, 1, lambda: [(one_index(), [(3000, 57)])]),
    "last_amp_plus_tiny": (12, 1, lambda: [(last_amp_plus_tiny(), [(3000, 58)])]),
    "shots_0_1_2": (10, 1, lambda: [(half_empty(), [(0, 59), (1, 59), (2, 59)])]),
    "unnormalised": (13, 1, lambda: [(unnormalised(), [(12000, 60)])]),
    "invalidation": (12, 1, _invalidation_steps),
}


# ---------------------------------------------------------------------------------------------------------------------
# programs for the tile-order path: the state is whatever qsv_exec leaves, the walk is that of its last pass
# ---------------------------------------------------------------------------------------------------------------------
def rand_u(seed):
    rs = np.random.RandomState(seed)
    q, _ = np.linalg.qr(rs.randn(2, 2) + 1j * rs.randn(2, 2))
    return q


def _factor(rs, k):
    return np.exp(1j * rs.randn(2 ** k)) * (0.5 + rs.rand(2 ** k))


def _distinct_diagonals(rs, W, skip=()):
    """diagonal factors of non-unit modulus over every qubit not in ``skip``, four at a time: every |amp| distinct"""
    from qcmrf_amd import ir
    qs = [q for q in range(W) if q not in skip]
    return [ir.op_diag(qs[i:i + 4], _factor(rs, len(qs[i:i + 4]))) for i in range(0, len(qs), 4)]


def general_and_table(trailing_x=()):
    """W = 16.  init without qubits 11 and 15, diagonals, a dense 2x2 that populates qubit 11 (15 stays |0>: under zero
    tracking the last pass walks half the tiles), controlled 2x2 (general passes), multiplexed 2x2 (table passes); the
    last two ops share a target, so that the program ends in a pass of more than one op at every tile width"""
    from qcmrf_amd import ir
    W = 16
    rs = np.random.RandomState(71)
    ops = [ir.op_init((1 << W) - 1 - (1 << 11) - (1 << 15))] + _distinct_diagonals(rs, W, skip=(11, 15))
    ops.append(ir.op_u(11, rand_u(1)))
    ops.append(ir.op_u(9, rand_u(2), [3], [1]))
    ops.append(ir.op_u(12, rand_u(3), [7, 1], [0, 1]))
    ops.append(ir.op_mux([14, 2], 6, [rand_u(10 + k) for k in range(4)]))
    ops.append(ir.op_mux([15], 10, [rand_u(20 + k) for k in range(2)]))
    ops.append(ir.op_mux([13], 6, [rand_u(30 + k) for k in range(2)]))
    ops.append(ir.op_mux([14], 6, [rand_u(40 + k) for k in range(2)]))
    return ops + [ir.op_x(q) for q in trailing_x]


def init_pass_with_x():
    """W = 16, one write-only pass: init, diagonals, X on a block bit and on a lane bit, two multiplexed 2x2.  A pass
    that reads nothing may store through the X frame on every bit, block bits included."""
    from qcmrf_amd import ir
    W = 16
    rs = np.random.RandomState(72)
    ops = [ir.op_init((1 << W) - 1 - (1 << 15))] + _distinct_diagonals(rs, W, skip=(15,))
    ops += [ir.op_x(15), ir.op_x(1)]
    ops.append(ir.op_mux([13], 6, [rand_u(50 + k) for k in range(2)]))
    ops.append(ir.op_mux([14], 6, [rand_u(60 + k) for k in range(2)]))
    return ops


def generator_only(P):
    """W = 16: init plus diagonal factors, nothing else (the k_init_prod generator), the top LOCAL qubit left |0>"""
    from qcmrf_amd import ir
    W = 16
    top = W - (P.bit_length() - 1) - 1
    rs = np.random.RandomState(73 + P)
    return [ir.op_init((1 << W) - 1 - (1 << top))] + _distinct_diagonals(rs, W, skip=(top,)) + \
           [ir.op_diag([0, 5, 9], _factor(rs, 3)), ir.op_diag([2, 12], _factor(rs, 2))]


def four_super_blocks(x_top):
    """W = 22 at multi_r = 2: 4096 tiles, four super blocks of tile sums.  Qubit 21 is never populated: the upper half
    of the state is empty, or -- with an X on it in the first pass -- the lower half"""
    from qcmrf_amd import ir
    W = 22
    rs = np.random.RandomState(74)
    ops = [ir.op_init((1 << W) - 1 - (1 << 21))] + _distinct_diagonals(rs, W, skip=(21,))
    if x_top:
        ops.append(ir.op_x(21))
    ops.append(ir.op_mux([5], 8, [rand_u(70 + k) for k in range(2)]))
    ops.append(ir.op_mux([9], 8, [rand_u(72 + k) for k in range(2)]))
    ops.append(ir.op_mux([3], 12, [rand_u(74 + k) for k in range(2)]))
    ops.append(ir.op_mux([7], 12, [rand_u(76 + k) for k in range(2)]))
    ops.append(ir.op_mux([4], 10, [rand_u(78 + k) for k in range(2)]))
    ops.append(ir.op_mux([6], 10, [rand_u(80 + k) for k in range(2)]))
    return ops


# name -> (W, P, ops, shots, seed)
TILE_PROGRAMS = {
    "general_and_table": (16, 1, general_and_table, 10000, 81),
    "general_and_table_70000_shots": (16, 1, general_and_table, 70000, 96),
    "trailing_x_register_bit": (16, 1, lambda: general_and_table(trailing_x=(6,)), 10000, 82),
    "trailing_x_lane_bit": (16, 1, lambda: general_and_table(trailing_x=(1,)), 10000, 83),
    "trailing_x_block_bit": (16, 1, lambda: general_and_table(trailing_x=(15,)), 10000, 84),
    "init_pass_with_x": (16, 1, init_pass_with_x, 10000, 95),
    "generator_P1": (16, 1, lambda: generator_only(1), 10000, 86),
    "generator_P2": (16, 2, lambda: generator_only(2), 10000, 87),
    "four_super_blocks_upper_empty": (22, 1, lambda: four_super_blocks(False), 20000, 208),
    "four_super_blocks_lower_empty": (22, 1, lambda: four_super_blocks(True), 20000, 279),
}

_REFERENCE = {}


def tile_reference(name):
    """(records, data, amplitudes of the numpy engine) of a tile program, computed once per process"""
    if name not in _REFERENCE:
        from oracle.sharded_numpy import NumpyEngine
        from qcmrf_amd import program
        W, P, ops, _, _ = TILE_PROGRAMS[name]
        rec, data = program.encode(ops())
        ref = NumpyEngine(W, P)
        ref.exec(rec, data)
        want = ref.amplitudes()
        want.setflags(write=False)
        _REFERENCE[name] = (rec, data, want)
    return _REFERENCE[name]
