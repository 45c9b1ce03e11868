"""The density-matrix method (``qsv_density_*``, ``run(method="density_matrix")``): numpy reference, stand-in engine and the
cases of the device tests (test infrastructure).

Convention (include/qsv.h): rho of W qubits is the vector of a 2W-qubit engine, rho[i, j] at v = i | (j << W).

  numpy_rho               the whole rho of a record stream, by the walkers of ``_density_matrix`` / ``_kraus_reference``
  vec_of                  rho -> the engine's vector
  exact_density_sample    what ``density_sample`` returns, word by word, from a diagonal: P_i = max(Re rho_ii, 0),
                          u = u01(seed, shot, 1, 0), ``pick_basis_state``, ``record_words``
  DensityNumpyEngine      the three entry points on numpy: the stand-in engine of the host tests
  pair_program            W = 12, 13: entanglement confined to fixed disjoint pairs, so rho is a Kronecker product of 2 x 2 and
                          4 x 4 factors and the reference costs nothing
  pair_program_k2         the same with KRAUS2 records inside the pairs (factors by ``_kraus2_reference.kraus2_rho``): the
                          programs of test_gpu_density_forms.py at W = 6 .. 16, with the wrong references of its host tests
"""
from __future__ import annotations

import functools

import numpy as np

import _kraus2_cases as k2c
import _kraus_cases as kc
import _noise_exact_cases as nc
from _density_matrix import _gate_rows, _init_vector, _pauli_channel, _pauli_probs, _records, word_distribution
from _kraus2_reference import kraus2_rho
from _kraus_reference import _apply_2x2, kraus_of_record
from _philox_reference import STREAM_SAMPLE, TOL, pick_basis_state, record_words, u01
from qcmrf_amd import _lib, ir, program

WIDTHS = (1, 2, 3, 5, 6, 7, 10)
WIDTH_INIT = {1: "zero", 2: None, 3: "uniform", 5: None, 6: "mid", 7: "uniform", 10: "mid"}
WIDTH_RANDOM = {1: 24, 2: 24, 3: 24, 5: 24, 6: 24, 7: 20, 10: 6}     # records of the random part: the numpy rho of W = 10 costs 16 MiB a copy


def numpy_rho(rec, data, W):
    """rho after the record stream from |0..0><0..0|: U rho U^dg, sum_p P(p) P rho P^dg, sum_k K_k rho K_k^dg"""
    N = 1 << W
    rho = np.zeros((N, N), dtype=np.complex128)
    rho[0, 0] = 1.0
    data = np.ascontiguousarray(data, dtype=np.float64)
    for kind, t, qs, vs, off, mask, angle in _records(rec, data):
        if kind in (_lib.OP_INIT_ZERO, _lib.OP_INIT_UNIFORM):
            v = _init_vector(N, kind, mask)
            rho = np.outer(v, v.conj())
        elif kind == _lib.OP_PAULI:
            rho = _pauli_channel(rho, qs, _pauli_probs(data, off, len(qs)))
        elif kind == _lib.OP_KRAUS:
            K, _ = kraus_of_record(data, off, vs[0])
            new = np.zeros_like(rho)
            for k in K:
                a = _apply_2x2(rho, qs[0], k)
                new += _apply_2x2(a.conj().T.copy(), qs[0], k).conj().T
            rho = new
        else:
            a = _gate_rows(rho.copy(), kind, t, qs, vs, off, mask, angle, data)
            rho = _gate_rows(a.conj().T.copy(), kind, t, qs, vs, off, mask, angle, data)    # U (U rho)^dg = U rho U^dg, rho Hermitian
    return rho


def mirrored_rho(rec, data, W):
    """rho by the convention of the engine: the vector of 2W qubits, every unitary record applied as itself on the ket bits
    and as its mirror on the bra bits (two in-place updates of one vector: much cheaper than ``numpy_rho`` on long
    programs), the channels on its (j, i) matrix view, which holds rho^T: a Pauli channel commutes with the transpose,
    a Kraus channel acts there with conj(K)"""
    N = 1 << W
    vec = np.zeros((N * N, 1), dtype=np.complex128)
    vec[0] = 1.0
    data = np.ascontiguousarray(data, dtype=np.float64)
    cdata = data.copy()
    cdata[1::2] *= -1.0                                             # tables start at even offsets: (re, im) pairs conjugated
    for kind, t, qs, vs, off, mask, angle in _records(rec, data):
        if kind in (_lib.OP_INIT_ZERO, _lib.OP_INIT_UNIFORM):
            m = 0 if kind == _lib.OP_INIT_ZERO else mask
            vec[:, 0] = _init_vector(N * N, _lib.OP_INIT_UNIFORM, m | (m << W))
        elif kind == _lib.OP_PAULI:
            vec = np.ascontiguousarray(_pauli_channel(vec.reshape(N, N), qs, _pauli_probs(data, off, len(qs)))).reshape(-1, 1)
        elif kind == _lib.OP_KRAUS:
            K, _ = kraus_of_record(data, off, vs[0])
            A = vec.reshape(N, N)
            new = np.zeros_like(A)
            for k in K.conj():
                a = _apply_2x2(A, qs[0], k)
                new += _apply_2x2(a.conj().T.copy(), qs[0], k).conj().T
            vec = np.ascontiguousarray(new).reshape(-1, 1)
        else:
            vec = _gate_rows(vec, kind, t, qs, vs, off, mask, angle, data)
            vec = _gate_rows(vec, kind, t + W, [q + W for q in qs], vs, off, mask, -angle, cdata)
    return vec.reshape(N, N).T


def vec_of(rho):
    """vector index v = i | (j << W): j is the slow index"""
    return np.ascontiguousarray(rho.T).reshape(-1)


def marginal(diag, qubits):
    """sum of diag over the i whose bits qubits[b] spell j (not clipped)"""
    idx = np.arange(diag.size)
    j = np.zeros(diag.size, dtype=np.int64)
    for b, q in enumerate(qubits):
        j |= ((idx >> q) & 1) << b
    return np.bincount(j, weights=diag, minlength=1 << len(qubits))


def exact_density_sample(diag, shots, seed, meas_qubits=None, readout=None, first_shot=0, tol=TOL):
    """(words, alt_words, ambiguous) of ``density_sample`` on a state with the diagonal ``diag``"""
    seed = int(seed) & (2 ** 64 - 1)
    shot = np.arange(int(shots), dtype=np.uint64) + np.uint64(first_shot)
    prob = np.repeat(np.clip(np.asarray(diag, dtype=np.float64), 0.0, None)[:, None], 1, axis=1)
    u = u01(seed, shot, STREAM_SAMPLE, 0)
    k = np.zeros(shot.size, dtype=np.uint64)
    alt = np.zeros(shot.size, dtype=np.uint64)
    amb = np.zeros(shot.size, dtype=bool)
    step = max(1, (1 << 22) // prob.shape[0])
    for lo in range(0, shot.size, step):
        hi = min(shot.size, lo + step)
        k[lo:hi], alt[lo:hi], amb[lo:hi] = pick_basis_state(np.broadcast_to(prob, (prob.shape[0], hi - lo)), u[lo:hi], tol)
    return record_words(k, seed, shot, meas_qubits, readout), record_words(alt, seed, shot, meas_qubits, readout), amb


class DensityNumpyEngine:
    """``density_exec`` / ``density_diagonal`` / ``density_sample`` of qcmrf_amd._lib.Engine on numpy, to the contract in
    include/qsv.h.  ``free_bytes`` is what ``device_memory`` reports (the backend's memory refusal reads it)."""

    free_bytes = 1 << 40
    made = []

    def __init__(self, n_qubits, devices=(0,), rank=None, world_size=None):
        if n_qubits % 2:
            raise ValueError("a density matrix of W qubits takes an engine of 2W qubits, not %d" % n_qubits)
        self.n_qubits = int(n_qubits)
        self.W = self.n_qubits // 2
        self.rho = None
        self.calls = []
        DensityNumpyEngine.made.append(self)

    @staticmethod
    def device_memory(device=0):
        return DensityNumpyEngine.free_bytes, 288 << 30

    def density_exec(self, ops, data):
        for r in ops:
            if int(r["kind"]) in (_lib.OP_MUX, _lib.OP_KQ, _lib.OP_SWAP):
                raise RuntimeError("qsv (-5): kind %d is not supported by the density-matrix method" % int(r["kind"]))
        self.calls.append("density_exec")
        self.rho = mirrored_rho(ops, data, self.W)

    def density_diagonal(self, qubits):
        self.calls.append("density_diagonal")
        d = np.real(np.diag(self.rho))
        return marginal(d, list(qubits)), float(d.sum())

    def density_sample(self, shots, seed, meas_qubits=None, readout=None):
        self.calls.append("density_sample")
        return exact_density_sample(np.real(np.diag(self.rho)), shots, seed, meas_qubits, readout)[0]

    def amplitudes(self, start=0, count=None):
        v = vec_of(self.rho)
        return v[start:] if count is None else v[start:start + count]

    def noisy_sample(self, *a, **k):
        raise AssertionError("method='density_matrix' must not reach noisy_sample")

    def exec(self, *a, **k):
        raise AssertionError("method='density_matrix' must not reach exec")

    def sync(self): pass
    def close(self): pass
    def set_option(self, name, value): pass
    def reset_stats(self): pass
    def set_profiling(self, on): pass


# ---- record-level cases of the device tests -------------------------------------------------------------------------------

def width_ops(W):
    """seeded random records of every accepted kind (``random_ops``: controlled 2x2, MCX, DIAG, MCPHASE, one- and two-qubit
    PAULI in both qubit orders, adjacent and not) with Kraus sets of m = 1..4 on the targets 0, 5, W - 1 (``with_kraus``)"""
    rng = np.random.RandomState(9000 + W)
    ops = nc.random_ops(W, 7000 + W, n_random=WIDTH_RANDOM[W], init=WIDTH_INIT[W])
    if W == 10:                                                     # fewer channels: every record walks 2^20 elements in numpy
        ops = [o for i, o in enumerate(ops) if o.kind != "diag" or i % 2 == 0]
        head = next(i for i, o in enumerate(ops) if o.kind != "init") + W
        for q, m in ((0, 2), (5, 3), (W - 1, 4), (5, 1)):
            ops.insert(int(rng.randint(head, len(ops) + 1)), kc.kraus_op(q, kc.isometry_kraus(rng, m)))
        return ops
    return kc.with_kraus(ops, W, rng)


@functools.lru_cache(maxsize=None)
def width_case(W):
    """(rec, data, rho) of a width; rho computed once, shared, left unchanged"""
    rec, data = program.encode(width_ops(W))
    rho = numpy_rho(rec, data, W)
    rho.setflags(write=False)
    return rec, data, rho


def w11_ops():
    """W = 11: the bra bit of qubit 0 is address bit 11.  Few records (the numpy rho is 64 MiB a copy): every channel kind
    on qubit 0, a two-qubit PAULI across the register"""
    rng = np.random.RandomState(1111)
    W = 11
    ops = [ir.op_init(0b10000100001), ir.op_u(0, nc._unitary(rng)), ir.op_x(0, [10], [1]), nc._pauli(rng, [0]),
           kc.kraus_op(0, kc.isometry_kraus(rng, 2)), nc._pauli(rng, [10, 0])]
    return ops, W


@functools.lru_cache(maxsize=None)
def w11_case():
    ops, W = w11_ops()
    rec, data = program.encode(ops)
    rho = numpy_rho(rec, data, W)
    rho.setflags(write=False)
    return rec, data, rho


# ---- sampling cases: (W, rec, data, shots, seed, meas, readout) -------------------------------------------------------------

def noise_free_case():
    """no PAULI and no KRAUS record: ``density_sample`` and ``noisy_sample`` must agree word for word"""
    W = 6
    ops = [o for o in nc.random_ops(W, 6600, n_random=30, init="uniform") if o.kind != "pauli"]
    rec, data = program.encode(ops)
    ro = np.tile([0.03, 0.06], (W + 1, 1))
    return dict(W=W, rec=rec, data=data, shots=2000, seed=2 ** 33 + 3, meas=[3, 0, -1, 5, 1, 2, 4], readout=ro)


SAMPLE_CASES = {"mapping 64 bits": nc.mapping_case, "noise free": noise_free_case, "prefix of 6000": functools.partial(kc.seed_case, kc.BIG_SEEDS[0], 6000)}
SAMPLE_CASES.update({"seed %#x" % s: functools.partial(kc.seed_case, s) for s in nc.SEEDS})


@functools.lru_cache(maxsize=None)
def sample_case(name):
    return SAMPLE_CASES[name]()


@functools.lru_cache(maxsize=None)
def sample_reference(name):
    """(words, alt_words, ambiguous, diagonal) of a named sampling case: computed once, shared, left unchanged"""
    c = sample_case(name)
    diag = np.real(np.diag(numpy_rho(c["rec"], c["data"], c["W"])))
    ref = exact_density_sample(diag, c["shots"], c["seed"], c["meas"], c["readout"]) + (diag,)
    for a in ref:
        a.setflags(write=False)
    return ref


# ---- W = 12, 13: products of pair factors -----------------------------------------------------------------------------------

PAIRS = ((0, -1), (5, 6), (-2, 7))          # negative: counted from W (W - 1, W - 2); the other qubits stand alone


def pair_program(W, seed=1213):
    """(ops, factors): one-qubit gates and channels anywhere, cx and two-qubit PAULI inside a pair only.  ``factors`` is a
    list of (qubits, rho of that factor as a 2^k x 2^k matrix over those qubits, qubits[0] the low bit)."""
    rng = np.random.RandomState(seed)
    pairs = [tuple(q % W for q in p) for p in PAIRS]
    paired = {q for p in pairs for q in p}
    groups = pairs + [(q,) for q in range(W) if q not in paired]
    per, factors = [], []
    for n, g in enumerate(groups):
        k = len(g)
        mk = []                                                     # each record as a function of the group's qubits
        for j in range(k):
            mk.append(lambda q, j=j, u=nc._unitary(rng): ir.op_u(q[j], u))
        if k == 2:
            mk.append(lambda q: ir.op_x(q[1], [q[0]], [1]))
            mk.append(lambda q, t=rng.dirichlet(np.ones(16)): ir.Op("pauli", qubits=(q[0], q[1]), table=t))
            mk.append(lambda q, u=nc._unitary(rng): ir.op_u(q[0], u))
            mk.append(lambda q: ir.op_x(q[0], [q[1]], [0]))
            mk.append(lambda q, t=rng.dirichlet(np.ones(16)): ir.Op("pauli", qubits=(q[1], q[0]), table=t))
        mk.append(lambda q, ks=kc.isometry_kraus(rng, 1 + n % 4): kc.kraus_op(q[0], ks))
        if n % 3 == 0:
            mk.append(lambda q, t=rng.dirichlet(np.ones(4)): ir.Op("pauli", qubits=(q[k - 1],), table=t))
        rec, data = program.encode([f(list(range(k))) for f in mk])
        factors.append((g, numpy_rho(rec, data, k)))
        per.append([f(g) for f in mk])
    order = rng.permutation(len(groups))                            # interleave the groups, the order inside a group kept
    out = []
    while any(per):
        for gi in order:
            if per[gi]:
                out.append(per[gi].pop(0))
    return out, factors


def product_entries(factors, W, rows, cols):
    """rho[rows, cols] (elementwise over two index arrays) of the Kronecker product"""
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    out = np.ones(np.broadcast(rows, cols).shape, dtype=np.complex128)
    for g, f in factors:
        a = np.zeros_like(rows)
        b = np.zeros_like(cols)
        for k, q in enumerate(g):
            a |= ((rows >> q) & 1) << k
            b |= ((cols >> q) & 1) << k
        out = out * f[a, b]
    return out


def product_diagonal(factors, W):
    i = np.arange(1 << W)
    return np.real(product_entries(factors, W, i, i))


# ---- W = 6 .. 16: products of pair factors with KRAUS2 records ---------------------------------------------------------------

# negative: counted from W.  (0, W - 1): bra bits W and 2W - 1; an adjacent low pair; where W allows (W <= 11) a qubit whose bra
# bit is address bit 11: qubit 5 at W = 6, qubit 4 at W = 7, qubit 0 at W = 11
K2_PAIRS = {6: ((0, -1), (2, 3), (4, 1)), 7: ((0, -1), (5, 2), (1, 4)), 11: ((0, -1), (5, 6), (2, 8)), 13: PAIRS, 14: PAIRS,
            16: ((0, -1), (5, 6))}
K2_SEED = 1600
# ways the engine could be wrong that the comparison with the factors must see (``wrong``; the program stays the true one):
# the first KRAUS2 record of the pair (0, W - 1) with its two qubits swapped, every Kraus operator conjugated, rho transposed
# (ket and bra exchanged), the factor of the pair (0, W - 1) left without its channels
K2_WRONG = ("swapped", "conjugated", "transposed", "no_channel")
CHANNELS = ("pauli", "kraus", "kraus2")


def _wrong_records(sub, wrong, n):
    if wrong == "swapped" and n == 0:
        i = next(i for i, o in enumerate(sub) if o.kind == "kraus2")
        sub = sub[:i] + [k2c.kraus2_op(sub[i].qubits[1], sub[i].qubits[0], sub[i].table)] + sub[i + 1:]
    elif wrong == "conjugated":
        sub = [ir.Op(o.kind, qubits=o.qubits, table=o.table.conj()) if o.kind in ("kraus", "kraus2") else o for o in sub]
    elif wrong == "no_channel" and n == 0:
        sub = [o for o in sub if o.kind not in CHANNELS]
    return sub


def pair_program_k2(W, pairs, seed, short=False, wrong=None):
    """(ops, factors) as ``pair_program``, from |+>^W (an INIT_UNIFORM record: every entry of rho has weight before the first
    gate), with KRAUS2 records inside the pairs: on (q0, q1), on (q1, q0) and on (q0, q1) again, cycling through the stacks
    of ``_kraus2_cases.menu`` (three pairs: all eight, m = 16 and the correlated damping sets included), two-qubit PAULI in
    both orders, one-qubit KRAUS of m = 1..4 and PAULI records, the entangling gates of ``pair_program``.
    ``short``: at most 16 records for the widths where a record is a sweep of many GiB -- gates on the paired qubits only,
    one KRAUS2 (the first of one operator, the second of two) and one two-qubit PAULI per pair, a one-qubit KRAUS and a
    PAULI on each qubit of the first pair.  ``wrong`` (one of K2_WRONG) changes the factors alone."""
    if wrong is not None and wrong not in K2_WRONG:
        raise ValueError("unknown wrong reference %r" % (wrong,))
    rng = np.random.RandomState(seed)
    stacks = k2c.menu(rng)
    pairs = [tuple(q % W for q in p) for p in pairs]
    paired = {q for p in pairs for q in p}
    assert len(paired) == 2 * len(pairs)
    groups = pairs + [(q,) for q in range(W) if q not in paired]
    n_k2 = [0]

    def k2(a, b):
        st = stacks[n_k2[0] % len(stacks)]
        n_k2[0] += 1
        return lambda q: k2c.kraus2_op(q[a], q[b], st)

    def pauli(n_qubits, *js):
        t = 0.3 * rng.dirichlet(np.ones(4 ** n_qubits))             # generic, the identity at 0.7 and more: as noise is, and a
        t[0] += 1.0 - t.sum()                                       # wrong record elsewhere is not depolarised out of sight
        return lambda q: ir.Op("pauli", qubits=tuple(q[j] for j in js), table=t)

    per, factors = [], []
    for n, g in enumerate(groups):
        k = len(g)
        mk = []                                                     # each record as a function of the group's qubits
        if k == 2 or not short:
            for j in range(k):
                mk.append(lambda q, j=j, u=nc._unitary(rng): ir.op_u(q[j], u))
        if k == 2:
            mk.append(lambda q: ir.op_x(q[1], [q[0]], [1]))
            mk.append(k2(0, 1))
            mk.append(pauli(2, 1, 0))
            if not short:
                mk.append(lambda q, u=nc._unitary(rng): ir.op_u(q[0], u))
                mk.append(lambda q: ir.op_x(q[0], [q[1]], [0]))
                mk.append(k2(1, 0))
                mk.append(pauli(2, 0, 1))
                mk.append(k2(0, 1))
        if short and n == 0:
            for j in (1, 0):
                mk.append(lambda q, j=j, ks=kc.isometry_kraus(rng, 2 + 2 * j): kc.kraus_op(q[j], ks))
                mk.append(pauli(1, 1 - j))
        elif not short:
            for j in range(k):
                mk.append(lambda q, j=j, ks=kc.isometry_kraus(rng, 1 + (n + j) % 4): kc.kraus_op(q[j], ks))
            if n % 3 == 0:
                mk.append(pauli(1, k - 1))
        sub = _wrong_records([ir.op_init((1 << k) - 1)] + [f(list(range(k))) for f in mk], wrong, n)
        rec, data = program.encode(sub)
        fac = kraus2_rho(rec, data, k)
        factors.append((g, fac.T.copy() if wrong == "transposed" else fac))
        per.append([f(g) for f in mk])
    order = rng.permutation(len(groups))                            # interleave the groups, the order inside a group kept
    out = [ir.op_init((1 << W) - 1)]
    while any(per):
        for gi in order:
            if per[gi]:
                out.append(per[gi].pop(0))
    return out, factors


@functools.lru_cache(maxsize=None)
def k2_case(W, short=False, seed=None):
    """dict(W, ops, rec, data, factors) of ``pair_program_k2(W, K2_PAIRS[W], K2_SEED + W)``: made once, shared, left unchanged"""
    ops, factors = pair_program_k2(W, K2_PAIRS[W], K2_SEED + W if seed is None else seed, short)
    rec, data = program.encode(ops)
    for _, f in factors:
        f.setflags(write=False)
    return dict(W=W, ops=ops, rec=rec, data=data, factors=factors)


def k2_wrong_factors(W, wrong, short=False):
    return pair_program_k2(W, K2_PAIRS[W], K2_SEED + W, short, wrong)[1]


def column_set(W):
    """the columns rho[:, j] the wide tests read: j = 0, 2^W - 1, every single bit (each bra bit of the address both ways, the
    top one -- address bit 2W - 1 -- included) and 16 seeded random j"""
    rng = np.random.RandomState(4000 + W)
    return [0, (1 << W) - 1] + [1 << b for b in range(W)] + [int(j) for j in rng.randint(1 << W, size=16)]


def product_columns(factors, W, cols):
    """(len(cols), 2^W): row c is rho[:, cols[c]], what ``amplitudes(cols[c] << W, 1 << W)`` reads"""
    return product_entries(factors, W, np.arange(1 << W)[None, :], np.asarray(cols, dtype=np.int64)[:, None])


def product_vector(factors, W, block=64):
    """the engine's whole vector (v = i | (j << W)) of the Kronecker product, built column block by column block"""
    N = 1 << W
    out = np.empty(N * N, dtype=np.complex128)
    for lo in range(0, N, block):
        out[lo * N:(lo + block) * N] = product_columns(factors, W, np.arange(lo, min(N, lo + block))).reshape(-1)
    return out


@functools.lru_cache(maxsize=None)
def k2_vector(W):
    """the reference vector of ``k2_case(W)``: computed once, shared, left unchanged (64 MiB at W = 11)"""
    v = product_vector(k2_case(W)["factors"], W)
    v.setflags(write=False)
    return v


# ---- sampling past the grid cap of the per-shot kernel (4096 workgroups of 256 threads = 2^20 shots) ---------------------------

def big_sample_case():
    """W = 2: a short noisy program, 2^20 + 777 shots, a seed above 2^32, a permuted register with an unused bit, readout errors"""
    rng = np.random.RandomState(2020)
    ops = [ir.op_u(0, nc._unitary(rng)), ir.op_u(1, nc._unitary(rng)), ir.op_x(1, [0], [1]),
           k2c.kraus2_op(1, 0, k2c.isometry_kraus2(rng, 2)), nc._pauli(rng, [0, 1]), kc.kraus_op(1, kc.isometry_kraus(rng, 2))]
    rec, data = program.encode(ops)
    ro = np.array([[0.03, 0.05], [0.2, 0.1], [0.0, 0.07]])
    return dict(W=2, rec=rec, data=data, shots=2 ** 20 + 777, seed=2 ** 35 + 5, meas=[1, -1, 0], readout=ro)


@functools.lru_cache(maxsize=None)
def big_sample_reference():
    """(case, words, alt_words, ambiguous, diagonal): computed once, shared, left unchanged"""
    c = big_sample_case()
    diag = np.real(np.diag(kraus2_rho(c["rec"], c["data"], c["W"])))
    ref = exact_density_sample(diag, c["shots"], c["seed"], c["meas"], c["readout"]) + (diag,)
    for a in ref:
        a.setflags(write=False)
    return (c,) + ref
