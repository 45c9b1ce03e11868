"""Programs of the tests of MEASURE records (test infrastructure).  ``GPU_CASES`` names every case the word-by-word GPU
tests run through ``check_measure_words``; the host tests walk the same dictionary to assert that the reference alone
stays within the ambiguity cap and to run the comparison against deliberately wrong references."""
from __future__ import annotations

import functools
import hashlib
import itertools
import os

import numpy as np

import _kraus_cases as kc
import _noise_exact_cases as nc
from _measure_reference import exact_measure_sample
from qcmrf_amd import QCMRF, ir, program
from qcmrf_amd.noise import ReadoutError
from qcmrf_amd.transpile import transpile

WIDTHS = (1, 2, 3, 6, 7, 8, 10, 11, 13)       # fewer amplitudes than lanes, one pair / eight pairs per lane, both thread counts, the full LDS
HBM_WIDTHS = (6, 10, 13)                      # the same cases through the slot path
WIDE_WIDTHS = (14, 16)                        # and what only the slot path holds
SLOTS = (0, 5, 6)                             # and W - 1
CLBITS = (0, 31, 32, 63)
FLIPS = ((0.0, 0.0), (1.0, 1.0), (0.1, 0.3), (0.0, 1.0), (0.25, 0.0), (1.0, 0.0), (0.02, 0.05), (0.5, 0.5))
SHOTS = 1500
# records between the MEASURE records: the reference evolves 2^W x 1500 amplitudes per record, so the wide cases keep few
N_RANDOM = {1: 32, 2: 32, 3: 32, 6: 32, 7: 32, 8: 24, 10: 8, 11: 6, 13: 4, 14: 8, 16: 8}
INIT = {1: "zero", 2: None, 3: "uniform", 6: "mid", 7: "uniform", 8: None, 10: "zero", 11: "uniform", 13: None,
        14: "uniform", 16: None}
WIDE_SHOTS = {14: 48, 16: 12}                 # the shot counts of _wide_reference


def slots(W):
    return sorted({q for q in SLOTS + (W - 1,) if q < W})


def measure_op(slot, clbit, release, flips):
    return ir.Op("measure", target=int(slot), mask=int(clbit), vals=(int(release),), table=None if flips is None else tuple(flips))


def with_measures(ops, W, rng):
    """``ops`` with MEASURE records spliced in at random places behind the first layer: every slot of ``slots(W)`` with
    release 0 and 1, at least 8 records, the classical bits of CLBITS in turn (so each is written twice: the second record
    overwrites), the flips of FLIPS in turn.  Gates that follow act on the measured and on the released slots."""
    ops = list(ops)
    head = next(i for i, o in enumerate(ops) if o.kind != "init") + W
    combos = list(itertools.product(slots(W), (1, 0)))
    while len(combos) < 8:
        combos += combos
    for i, (s, release) in enumerate(combos):
        ops.insert(int(rng.randint(head, len(ops) + 1)), measure_op(s, CLBITS[i % 4], release, FLIPS[i % len(FLIPS)]))
    return ops


def register(W, rng):
    """a 64-bit register: the bits of CLBITS belong to the MEASURE records (-1), a few others read qubits at the end"""
    meas = [-1] * 64
    ro = np.zeros((64, 2))
    for j in (1, 2, 5, 30, 33, 40, 62):
        meas[j] = int(rng.randint(W))
        ro[j] = rng.uniform(0.0, 0.3, 2)
    ro[list(CLBITS)] = 1.0                                           # a final flip that must not happen
    return meas, ro


def random_case(W, shots=SHOTS):
    rng = np.random.RandomState(7000 + W)
    base = nc.random_ops(W, 7100 + W, n_random=N_RANDOM[W], init=INIT[W])
    for q in slots(W)[:2]:                                           # Kraus records among them: the kinds share one op
        base.insert(int(rng.randint(W + 1, len(base) + 1)), kc.kraus_op(q, kc.isometry_kraus(rng, 1 + q % 4)))
        base.insert(int(rng.randint(W + 1, len(base) + 1)), kc.kraus_op(q, kc.constructor_kraus(rng, q % 4)))
    rec, data = program.encode(with_measures(base, W, rng))
    meas, ro = register(W, rng)
    return dict(W=W, rec=rec, data=data, shots=shots, seed=7700 + W, meas=meas, readout=ro)


def wide_case(W):
    return random_case(W, WIDE_SHOTS[W])


def grid_case(shots=SHOTS):
    """W = 4 with a seed above 2^32 and a state whose mass is not 1, for grids, partial rounds and prefixes"""
    c = dict(random_case_w4())
    c.update(shots=shots)
    return c


@functools.lru_cache(maxsize=None)
def random_case_w4():
    W = 4
    rng = np.random.RandomState(7404)
    ops = kc.with_kraus(nc.random_ops(W, 7444, n_random=24), W, rng)
    ops.insert(W, ir.op_diag([1], [0.6, 0.9]))                      # the state's mass is not 1 from here on: draws scale by it
    rec, data = program.encode(with_measures(ops, W, rng))
    meas, ro = register(W, rng)
    return dict(W=W, rec=rec, data=data, shots=SHOTS, seed=2 ** 32 + 77, meas=meas, readout=ro)


# ---- through the host path ------------------------------------------------------------------------------------------------

def chain(n):
    return [[i, i + 1] for i in range(n - 1)]


def chain_theta(n, seed=11):
    rng = np.random.RandomState(seed)
    return (-np.abs(rng.randn(sum(2 ** len(c) for c in chain(n)))) * 0.5).tolist()


def chain_circuit(n, lowered=True, seed=11):
    qc = QCMRF(chain(n), chain_theta(n, seed), with_measurements=True)
    return transpile(qc, basis_gates=nc.BASIS) if lowered else qc


def two_triangles(lowered=True, seed=12):
    rng = np.random.RandomState(seed)
    C = [[0, 1, 2], [2, 3, 4]]
    qc = QCMRF(C, (-np.abs(rng.randn(16)) * 0.5).tolist(), with_measurements=True)
    return transpile(qc, basis_gates=nc.BASIS) if lowered else qc


def many_cliques(n=6, m=20, seed=13):
    """n variables on m pair cliques, constructed: n + m + 1 = 27 qubits deferred, n + 2 live"""
    rng = np.random.RandomState(seed)
    pairs = [(a, b) for a in range(n) for b in range(a + 1, n)]
    C = [list(pairs[i % len(pairs)]) for i in rng.permutation(m)]
    return QCMRF(C, (-np.abs(rng.randn(4 * m)) * 0.5).tolist(), with_measurements=True)


def local_readout_model(nm, n=12):
    """readout errors that differ from qubit to qubit: a flip taken from the slot instead of the logical qubit shows"""
    for q in range(n):
        nm.add_readout_error(ReadoutError([[1.0 - 0.01 * (q + 1), 0.01 * (q + 1)], [0.02 * (q + 1), 1.0 - 0.02 * (q + 1)]]), [q])
    return nm


def lowered_model():
    """thermal relaxation, depolarizing and readout errors on the basis gates"""
    return kc.thermal_model()


def constructed_model():
    """the model of test_gpu_kraus.py's constructed case -- on the gate names a constructed circuit carries -- plus readout"""
    return kc.constructed_model()


def in_place_case(qc, nm, seed, shots):
    """a circuit under a noise model as ``run(noisy_measure="in_place")`` hands it to the engine"""
    from qcmrf_amd.backend import QsvBackend
    ing, rec, data, clist, meas, readout, _, state, (mode, width, n_measure) = QsvBackend._prepare_noisy(qc, nm, "auto", "in_place")
    assert mode == "in_place"
    return dict(W=width, rec=rec, data=data, shots=shots, seed=seed, meas=meas, readout=readout if ing.readout else None,
                state=state, n_measure=n_measure)


GPU_CASES = {"lds W=%d" % W: functools.partial(random_case, W) for W in WIDTHS}
GPU_CASES.update({"wide W=%d" % W: functools.partial(wide_case, W) for W in WIDE_WIDTHS})
GPU_CASES["grids"] = grid_case
GPU_CASES["prefix of 4000"] = functools.partial(grid_case, 4000)
GPU_CASES["6 variables, 20 cliques"] = lambda: in_place_case(many_cliques(), constructed_model(), 620, SHOTS)
GPU_CASES["chain(12)"] = lambda: in_place_case(chain_circuit(12, lowered=False), constructed_model(), 1212, 256)


@functools.lru_cache(maxsize=None)
def case(name):
    return GPU_CASES[name]()


def reference_of(c, **kw):
    return exact_measure_sample(c["rec"], c["data"], c["W"], c["shots"], c["seed"], c["meas"], c["readout"], **kw)


# The references of these cases evolve 2^W x shots amplitudes through every record in numpy, 15 s to minutes each, so their
# results are recorded under tests/golden/measure_refs/ (tests/golden/make_measure_refs.py writes them with
# ``exact_measure_sample``) together with a digest of everything that went in; test_measure_reference.py recomputes the
# first shots of each on every run, so a recorded file can neither go stale nor differ from the reference unnoticed.
RECORDED = {"lds W=11": 64, "lds W=13": 16, "6 variables, 20 cliques": 48, "chain(12)": 4}     # name -> shots recomputed
_REFS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "measure_refs")


def digest(c):
    """the integers a recorded reference depends on: every field of the records but the angle, the seed, the shots, the register"""
    h = hashlib.sha256()
    for f in ("kind", "target", "n", "flags", "qubits", "vals", "data_off", "mask"):
        h.update(np.ascontiguousarray(c["rec"][f]).tobytes())
    h.update(repr((c["W"], c["shots"], c["seed"], list(c["meas"]), c["readout"] is None)).encode())
    return h.hexdigest()


def floats(c):
    """and the floating-point numbers: angles, tables, flips.  Compared to 1e-12, not bit for bit: a library may round a
    sine or a QR factor differently on another CPU, and a difference that size moves no draw the reference calls determined"""
    ro = np.zeros(0) if c["readout"] is None else np.asarray(c["readout"], dtype=np.float64).ravel()
    return np.concatenate([np.asarray(c["rec"]["angle"], dtype=np.float64), np.asarray(c["data"], dtype=np.float64), ro])


def recorded_path(name):
    return os.path.join(_REFS, "".join(ch if ch.isalnum() else "_" for ch in name) + ".npz")


@functools.lru_cache(maxsize=None)
def reference(name):
    """(words, alt_words, ambiguous, undetermined) of a named case: computed (or read) once, shared, left unchanged"""
    if name in RECORDED:
        with np.load(recorded_path(name)) as f:
            stale = "%s: the recorded reference belongs to another program; run tests/golden/make_measure_refs.py" % name
            assert str(f["digest"]) == digest(case(name)), stale
            fl = floats(case(name))
            assert f["floats"].shape == fl.shape and np.abs(f["floats"] - fl).max() <= 1e-12, stale
            ref = tuple(f[k] for k in ("words", "alt_words", "ambiguous", "undetermined"))
    else:
        ref = reference_of(case(name))
    for a in ref:
        a.setflags(write=False)
    return ref


# ---- forced outcomes: plain equality, nothing of the Philox emulation involved --------------------------------------------

def forced_programs(W):
    """(label, (rec, data), meas, expected word): X, MEASURE with release, then a final measure of the same slot -- the
    recorded bit is 1 and the final bit 0 -- for every slot of ``slots(W)`` at once; the same with flips (1, 1) and
    (0, 0) spelled out; without release the final bit is 1 too; a bit overwritten by a second record"""
    ss = slots(W)
    meas = [-1] * 64
    for j, s in enumerate(ss):
        meas[8 + j] = s                                            # final bits 8.. read the slots again
    xs = [ir.op_x(s) for s in ss]
    early = lambda flips, release: [measure_op(s, j, release, flips) for j, s in enumerate(ss)]     # noqa: E731
    ones = sum(1 << j for j in range(len(ss)))
    finals = sum(1 << (8 + j) for j in range(len(ss)))
    yield "X, measure + release", program.encode(xs + early((0.0, 0.0), 1)), meas, ones
    yield "X, measure + release, flips (1, 1)", program.encode(xs + early((1.0, 1.0), 1)), meas, 0
    yield "measure |0>, flips (1, 1)", program.encode(early((1.0, 1.0), 1)), meas, ones
    yield "X, measure, no release", program.encode(xs + early((0.0, 0.0), 0)), meas, ones | finals
    yield "released slot flipped again", program.encode(xs + early((0.0, 0.0), 1) + xs), meas, ones | finals
    s = ss[-1]
    again = [ir.op_x(s), measure_op(s, 63, 1, (0.0, 0.0)), measure_op(s, 63, 0, (0.0, 0.0))]   # 1, then 0 over it
    yield "bit overwritten by a second record", program.encode(again), [-1] * 64, 0
    again = [measure_op(s, 63, 0, (0.0, 0.0)), ir.op_x(s), measure_op(s, 63, 1, (0.0, 0.0))]   # 0, then 1 over it
    yield "bit overwritten by a second record (1 last)", program.encode(again), [-1] * 64, 1 << 63
