"""MEASURE records on a density matrix (``qsv_density_exec_accept``, ``run(density_measure=...)``): reference, stand-in engine
and the cases of the device tests (test infrastructure).

The contract (include/qsv.h): a MEASURE record on qubit t with classical bit c, release flag and flips (f0, f1) maps every
2 x 2 block B over (ket bit t, bra bit t + W) to diag(w0 B00, w1 B11), with release to diag(w0 B00 + w1 B11, 0); w_b =
P(read v | true b) when c is in fix_mask (v = its bit of fix_val) and this record is the LAST that writes c, else w0 = w1 = 1.
The trace is not renormalised.

  reference_rho              rho as a 2^W x 2^W MATRIX, record by record; a MEASURE record as projectors:
                             w0 P0 rho P0 + w1 P1 rho P1 (release: the second term moved by X_t).  ``wrong`` (one of WRONG)
                             changes the rule the way an engine could get it wrong
  DensityMeasureNumpyEngine  the stand-in engine of the host tests: the engine's VECTOR of 2W qubits, a MEASURE record on the
                             two address bits t and t + W of its tensor view -- no line shared with the reference's rule
  kraus_twin                 the two-operator KRAUS record that is the same map (the device cross-check)
  width_case / w11_case      the record-level programs of the device tests, with their references (made once, shared)
"""
from __future__ import annotations

import functools
import itertools

import numpy as np

import _kraus2_cases as k2c
import _kraus_cases as kc
import _measure_cases as mc
import _noise_exact_cases as nc
from _density_cases import DensityNumpyEngine, vec_of
from _density_matrix import _gate_rows, _init_vector, _pauli_channel, _pauli_probs, _records
from _kraus2_reference import _apply_4x4, kraus2_of_record
from _kraus_reference import _apply_2x2, kraus_of_record
from _measure_reference import _conj_apply, measure_of_record
from qcmrf_amd import _lib, ir, program

WIDTHS = (1, 2, 3, 6, 7)                      # fewer blocks than lanes ... 4^7 / 4 = 4096 blocks: 16 workgroups of 256
NT_WIDTHS = (2, 3, 7)
N_RANDOM = {1: 16, 2: 16, 3: 16, 6: 12, 7: 8}
# seeds at which the accepted part keeps weight (trace > 1e-2: forced flips and repeated slots can leave none) and every
# wrong reference of WRONG moves some entry by more than 1e-4 (test_density_measure_host.py asserts both)
SEED = {1: 5101, 2: 5102, 3: 5103, 6: 5106, 7: 5117}
# the classical bits of the MEASURE records in turn: bits 0 and 31 are written twice
CLBITS = (0, 31, 32, 63, 7, 0, 31, 5)
FIX = {0: 1, 31: 0, 32: 1, 5: 0}              # fixed to 1, fixed to 0; 63 and 7 are forgotten
# ways an engine could be wrong that the comparison must see: f0 and f1 swapped, the slot not handed back in |0>,
# acceptance on the true bit instead of the bit as read, the earlier write of a twice-written bit conditioning too
WRONG = ("flips_swapped", "no_release", "true_bit", "early_write")


def mask_of(fix):
    fm = fv = 0
    for c, v in fix.items():
        fm |= 1 << c
        fv |= int(v) << c
    return fm, fv


def weights(c, flips, fm, fv, last, wrong=None):
    """(w0, w1) of a MEASURE record writing bit c; ``last``: it is the last record that writes c"""
    if not (fm >> c) & 1 or not (last or wrong == "early_write"):
        return 1.0, 1.0
    v = (fv >> c) & 1
    f = flips[::-1] if wrong == "flips_swapped" else flips
    if wrong == "true_bit":
        return float(v == 0), float(v == 1)
    return (1.0 - f[0] if v == 0 else f[0]), (1.0 - f[1] if v == 1 else f[1])


def last_writes(rec):
    last = {}
    for i, r in enumerate(rec):
        if int(r["kind"]) == _lib.OP_MEASURE:
            last[int(r["vals"][0])] = i
    return last


def measure_rho(rho, t, release, w0, w1):
    """the map on rho as a matrix: w0 P0 rho P0 + w1 P1 rho P1, release: w0 P0 rho P0 + w1 X P1 rho P1 X"""
    idx = np.arange(rho.shape[0])
    one = ((idx >> t) & 1).astype(bool)
    p0 = rho * np.outer(~one, ~one)
    p1 = rho * np.outer(one, one)
    if release:
        perm = idx ^ (1 << t)
        p1 = p1[np.ix_(perm, perm)]
    return w0 * p0 + w1 * p1


def reference_rho(rec, data, W, fix_mask=0, fix_val=0, wrong=None):
    """rho after the record stream of ``density_exec_accept`` from |0..0><0..0|, every record kind it takes"""
    if wrong is not None and wrong not in WRONG:
        raise ValueError("unknown wrong reference %r" % (wrong,))
    N = 1 << W
    rho = np.zeros((N, N), dtype=np.complex128)
    rho[0, 0] = 1.0
    data = np.ascontiguousarray(data, dtype=np.float64)
    last = last_writes(rec)
    for i, (r, (kind, t, qs, vs, off, mask, angle)) in enumerate(zip(rec, _records(rec, data))):
        if kind in (_lib.OP_INIT_ZERO, _lib.OP_INIT_UNIFORM):
            v = _init_vector(N, kind, mask)
            rho = np.outer(v, v.conj())
        elif kind == _lib.OP_PAULI:
            rho = _pauli_channel(rho, qs, _pauli_probs(data, off, len(qs)))
        elif kind == _lib.OP_KRAUS:
            K, _ = kraus_of_record(data, off, vs[0])
            rho = sum(_conj_apply(rho, lambda M, k=k: _apply_2x2(M, qs[0], k)) for k in K)
        elif kind == _lib.OP_KRAUS2:
            K, _ = kraus2_of_record(data, off, vs[0])
            rho = sum(_conj_apply(rho, lambda M, k=k: _apply_4x4(M, qs[0], qs[1], k)) for k in K)
        elif kind == _lib.OP_MEASURE:
            q, c, release, flips = measure_of_record(r, data)
            w0, w1 = weights(c, flips, fix_mask, fix_val, last[c] == i, wrong)
            rho = measure_rho(rho, q, release and wrong != "no_release", w0, w1)
        else:
            rho = _conj_apply(rho, lambda M: _gate_rows(M.copy(), kind, t, qs, vs, off, mask, angle, data))
    return rho


_PAULI = (np.eye(2, dtype=np.complex128), np.array([[0, 1], [1, 0]], dtype=np.complex128), np.diag([1.0 + 0j, -1.0]),
          np.array([[0, -1j], [1j, 0]]))          # index x | z << 1


def _superoperator(T, W, qubits, ks):
    """sum_k K rho K^dg on the tensor view T (address bit b on axis 2W - 1 - b) of the engine's vector: the ket and bra bits of
    ``qubits`` moved to the front, one matrix product with sum_k conj(K) (x) K (index: bra bits high, ket bits low, matrix
    index bit j of K on qubits[j])"""
    n = len(qubits)
    front = [2 * W - 1 - (q + W) for q in reversed(qubits)] + [2 * W - 1 - q for q in reversed(qubits)]
    S = sum(np.kron(k.conj(), k) for k in ks)
    A = np.moveaxis(T, front, list(range(2 * n)))
    shape = A.shape
    A = (S @ A.reshape(4 ** n, -1)).reshape(shape)
    return np.ascontiguousarray(np.moveaxis(A, list(range(2 * n)), front))


class DensityMeasureNumpyEngine(DensityNumpyEngine):
    """DensityNumpyEngine plus ``density_exec_accept``, on the engine's own convention and nothing else: the vector of 2W
    qubits, v = i | (j << W).  Unitary records run as themselves on the ket bits and mirrored on the bra bits, PAULI, KRAUS
    and KRAUS2 records as one superoperator on the ket and bra bits of their qubits, a MEASURE record on the address bits
    t and t + W.  ``density_exec`` is the same walk without MEASURE records (the parent's walks no KRAUS2 record and costs
    three transposes per Kraus operator)."""

    made = []

    def __init__(self, n_qubits, devices=(0,), rank=None, world_size=None):
        super().__init__(n_qubits, devices, rank, world_size)
        DensityMeasureNumpyEngine.made.append(self)

    def density_exec(self, ops, data):
        if any(int(r["kind"]) == _lib.OP_MEASURE for r in ops):
            raise RuntimeError("qsv (-5): QSV_OP_MEASURE runs in qsv_noisy_sample only; the density-matrix method defers every measurement")
        self._walk(ops, data, 0, 0)
        self.calls.append("density_exec")

    def density_exec_accept(self, ops, data, fix_mask=0, fix_val=0):
        if fix_val & ~fix_mask:
            raise ValueError("qsv (-1): fix_val sets a bit that fix_mask does not fix")
        self._walk(ops, data, fix_mask, fix_val)
        self.calls.append("density_exec_accept")

    def _walk(self, ops, data, fix_mask, fix_val):
        W, N = self.W, 1 << self.W
        vec = np.zeros((N * N, 1), dtype=np.complex128)
        vec[0] = 1.0
        data = np.ascontiguousarray(data, dtype=np.float64)
        cdata = data.copy()
        cdata[1::2] *= -1.0
        last = last_writes(ops)
        tensor = (2,) * (2 * W)
        for i, (r, (kind, t, qs, vs, off, mask, angle)) in enumerate(zip(ops, _records(ops, data))):
            if kind in (_lib.OP_INIT_ZERO, _lib.OP_INIT_UNIFORM):
                m = 0 if kind == _lib.OP_INIT_ZERO else mask
                vec[:, 0] = _init_vector(N * N, _lib.OP_INIT_UNIFORM, m | (m << W))
            elif kind == _lib.OP_PAULI:
                ks = []
                for p, pr in enumerate(_pauli_probs(data, off, len(qs))):
                    if pr > 0:
                        P = np.eye(1)
                        for j in range(len(qs)):
                            P = np.kron(_PAULI[(p >> (2 * j)) & 3], P)
                        ks.append(np.sqrt(pr) * P)
                vec = _superoperator(vec.reshape(tensor), W, qs, ks).reshape(-1, 1)
            elif kind == _lib.OP_KRAUS:
                vec = _superoperator(vec.reshape(tensor), W, qs, kraus_of_record(data, off, vs[0])[0]).reshape(-1, 1)
            elif kind == _lib.OP_KRAUS2:
                vec = _superoperator(vec.reshape(tensor), W, qs, kraus2_of_record(data, off, vs[0])[0]).reshape(-1, 1)
            elif kind == _lib.OP_MEASURE:
                q, c, release, flips = measure_of_record(r, data)
                if (fix_mask >> c) & 1 and last[c] == i:
                    v = (fix_val >> c) & 1
                    w = [(1.0 - flips[b]) if b == v else flips[b] for b in (0, 1)]
                else:
                    w = [1.0, 1.0]
                T = vec.reshape(tensor)                             # address bit b on axis 2W - 1 - b
                at = lambda a, b: tuple(a if ax == 2 * W - 1 - q else b if ax == 2 * W - 1 - (q + W) else slice(None) for ax in range(2 * W))   # noqa: E731
                b00, b11 = T[at(0, 0)].copy(), T[at(1, 1)].copy()
                T[at(0, 1)] = 0.0
                T[at(1, 0)] = 0.0
                T[at(0, 0)] = w[0] * b00 + (w[1] * b11 if release else 0.0)
                T[at(1, 1)] = 0.0 if release else w[1] * b11
            elif kind in (_lib.OP_MUX, _lib.OP_KQ, _lib.OP_SWAP):
                raise RuntimeError("qsv (-5): kind %d is not supported by the density-matrix method" % kind)
            else:
                vec = _gate_rows(vec, kind, t, qs, vs, off, mask, angle, data)
                vec = _gate_rows(vec, kind, t + W, [x + W for x in qs], vs, off, mask, -angle, cdata)
        self.rho = vec.reshape(N, N).T.copy()


def kraus_twin(t, release):
    """the KRAUS op of two operators |0><0| and |1><1| (release: |0><1|): scaled by sqrt(w0) and sqrt(w1) it is the map of a
    MEASURE record"""
    k0 = np.zeros((2, 2), dtype=np.complex128)
    k1 = np.zeros((2, 2), dtype=np.complex128)
    k0[0, 0] = 1.0
    k1[0 if release else 1, 1] = 1.0
    return kc.kraus_op(t, np.array([k0, k1]))


def with_twins(ops, fix):
    """(rec, data) of ``ops`` with every measure op replaced by its KRAUS twin under the fixed bits ``fix``: a program for
    ``density_exec``.  ``program.encode`` takes channels only, so the twins are encoded with weights 1 and their operators
    scaled by sqrt(w0), sqrt(w1) in the pool (the density-matrix method reads the operators alone, not the E tables)"""
    fm, fv = mask_of(fix)
    last = {}
    for i, o in enumerate(ops):
        if o.kind == "measure":
            last[int(o.mask)] = i
    rec, data = program.encode([kraus_twin(o.target, bool(o.vals[0])) if o.kind == "measure" else o for o in ops])
    data = np.array(data, dtype=np.float64)
    for i, o in enumerate(ops):
        if o.kind == "measure":
            c = int(o.mask)
            w0, w1 = weights(c, np.asarray(o.table, dtype=np.float64), fm, fv, last[c] == i)
            off = int(rec["data_off"][i])
            data[off:off + 8] *= np.sqrt(w0)
            data[off + 8:off + 16] *= np.sqrt(w1)
    return rec, data


def width_ops(W):
    """seeded random records of every unitary kind, PAULI, KRAUS and (W >= 2) KRAUS2, with at least 8 MEASURE records spliced
    in behind the first layer: every slot of {0, 5, 6, W - 1} with release 1 and 0, the flips of ``_measure_cases.FLIPS`` and
    the bits of CLBITS in turn"""
    rng = np.random.RandomState(SEED[W])
    ops = nc.random_ops(W, 100 + SEED[W], n_random=N_RANDOM[W], init=mc.INIT[W])
    head = next(i for i, o in enumerate(ops) if o.kind != "init") + W
    for q in mc.slots(W)[:2]:
        ops.insert(int(rng.randint(head, len(ops) + 1)), kc.kraus_op(q, kc.isometry_kraus(rng, 2 + q % 3)))
    for a, b in k2c.pairs(W)[:3]:
        ops.insert(int(rng.randint(head, len(ops) + 1)), k2c.kraus2_op(a, b, k2c.isometry_kraus2(rng, 2)))
    combos = list(itertools.product(mc.slots(W), (1, 0)))
    while len(combos) < 8:
        combos += combos
    for i, (s, release) in enumerate(combos):
        ops.insert(int(rng.randint(head, len(ops) + 1)), mc.measure_op(s, CLBITS[i % len(CLBITS)], release, mc.FLIPS[i % len(mc.FLIPS)]))
    return ops


@functools.lru_cache(maxsize=None)
def width_case(W):
    """dict(W, ops, rec, data, fix, rho): rho by ``reference_rho``, computed once, shared, left unchanged"""
    ops = width_ops(W)
    rec, data = program.encode(ops)
    rho = reference_rho(rec, data, W, *mask_of(FIX))
    rho.setflags(write=False)
    return dict(W=W, ops=ops, rec=rec, data=data, fix=dict(FIX), rho=rho)


def w11_ops():
    """W = 11, at most a dozen records (the numpy rho is 64 MiB a copy): MEASURE records with and without release on the
    slots 0, 5 and 10 -- fixed to 1, fixed to 0 and forgotten -- between a few gates and channels"""
    rng = np.random.RandomState(1112)
    ops = [ir.op_init(0b10000100001), ir.op_u(0, nc._unitary(rng)), ir.op_x(5, [10], [1]),
           mc.measure_op(0, 0, 1, (0.1, 0.3)), ir.op_u(0, nc._unitary(rng)), kc.kraus_op(10, kc.isometry_kraus(rng, 2)),
           mc.measure_op(10, 31, 0, (0.02, 0.05)), nc._pauli(rng, [5, 0]), mc.measure_op(5, 63, 1, (0.25, 0.0)),
           mc.measure_op(0, 32, 0, (0.25, 0.0))]
    return ops, 11


@functools.lru_cache(maxsize=None)
def w11_case():
    ops, W = w11_ops()
    rec, data = program.encode(ops)
    fix = {0: 1, 31: 0, 32: 1}
    rho = reference_rho(rec, data, W, *mask_of(fix))
    rho.setflags(write=False)
    return dict(W=W, ops=ops, rec=rec, data=data, fix=fix, rho=rho)


# ---- through run() ---------------------------------------------------------------------------------------------------------

def small_circuits():
    """(label, circuit, its post-selection, live width in place, width deferred)"""
    from qcmrf_amd import QCMRF
    yield "chain(3)", mc.chain_circuit(3), QCMRF(mc.chain(3), mc.chain_theta(3), with_measurements=True).post_selection(), 5, 6
    yield "chain(4)", mc.chain_circuit(4), QCMRF(mc.chain(4), mc.chain_theta(4), with_measurements=True).post_selection(), 6, 8
    yield "two triangles", mc.two_triangles(), mc.two_triangles(lowered=False).post_selection(), 7, 8


def small_model():
    return mc.local_readout_model(kc.thermal_model())


def as_array(probs, nbits):
    out = np.zeros(1 << nbits)
    for k, v in probs.items():
        out[int(k.replace(" ", ""), 2)] = v
    return out


def stand_in_backend(**options):
    from qcmrf_amd.backend import QsvBackend
    b = QsvBackend(**options)
    b._engine_factory = DensityMeasureNumpyEngine
    return b


@functools.lru_cache(maxsize=None)
def many_cliques_stand_in(model):
    """``run(many_cliques(), density_measure="in_place", accept=post_selection())`` on the stand-in engine: (probabilities as
    a dict, accept_probability, metadata).  ``model``: None or "constructed".  Made once, shared, left unchanged"""
    qc = mc.many_cliques()
    nm = mc.constructed_model() if model == "constructed" else None
    res = stand_in_backend().run(qc, shots=0, method="density_matrix", density_measure="in_place", accept=qc.post_selection(),
                                 noise_model=nm).result()
    return res.get_probabilities(), res.metadata(0)["accept_probability"], res.metadata(0)


def many_cliques_closed_form():
    """(Gibbs pmf over the 6 variables, success probability) of ``many_cliques()``"""
    from qcmrf_amd import mrf
    qc = mc.many_cliques()
    return mrf.gibbs_pmf(qc._cliques, qc.theta)[0], mrf.success_probability(qc._cliques, qc.theta)


def accept_probability_bound(model=None):
    """the relative bound on the device's accept_probability of ``many_cliques()``: 100 times the relative disagreement
    measured on the CPU between the stand-in engine and the closed form (two orders of margin for the device's other order
    of summation).  Under a noise model there is no closed form: the ideal case's bound holds there too, against the
    stand-in engine's number."""
    _, got, _ = many_cliques_stand_in(None)
    want = many_cliques_closed_form()[1]
    return 100.0 * abs(got - want) / want
