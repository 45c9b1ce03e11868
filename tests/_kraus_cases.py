"""Programs of the word-by-word tests of Kraus records (test infrastructure).  ``GPU_CASES`` names every case that
test_gpu_kraus_exact.py runs through ``check_kraus_words``; the host tests walk the same dictionary to assert that the
reference alone stays within the ambiguity cap (the seeds are fixed, so that is a property of the cases) and to run the
comparison against deliberately wrong references."""
from __future__ import annotations

import functools

import numpy as np

import _noise_exact_cases as nc
from _kraus_reference import exact_kraus_sample
from qcmrf_amd import QCMRF, ir, program
from qcmrf_amd.transpile import transpile
from qcmrf_amd.noise import (NoiseModel, ReadoutError, amplitude_damping_error, depolarizing_error, pauli_error,
                             phase_amplitude_damping_error, reset_error, thermal_relaxation_error)

WIDTHS = (1, 2, 3, 6, 7, 10, 11, 13)          # both thread counts, fewer amplitudes than lanes, the full LDS
TARGETS = (0, 5, 6, 7, 8)                     # and W - 1
BIG_SEEDS = (2 ** 32 + 7, 2 ** 63 + 12345)


def isometry_kraus(rng, m):
    """m generic Kraus operators: the 2 x 2 blocks of a random 2m x 2 isometry (sum K^dg K = 1); every branch has a
    weight of the order 1 / m"""
    q, _ = np.linalg.qr(rng.randn(2 * m, 2) + 1j * rng.randn(2 * m, 2))
    return q.reshape(m, 2, 2)


def _stack(err):
    (kind, _, ks), = err.terms()
    assert kind == "kraus"
    return ks


def constructor_kraus(rng, which, lo=0.05, hi=0.5):
    """the Kraus stack of one of the model's constructors with parameters in [lo, hi]"""
    a, b, p1 = rng.uniform(lo, hi), rng.uniform(lo, hi), rng.uniform(lo, hi)
    if which == 0:
        return _stack(amplitude_damping_error(a))
    if which == 1:
        return _stack(phase_amplitude_damping_error(a, b, p1))          # six operators reduced to four
    if which == 2:
        return _stack(reset_error(a, 0.5 * b))                          # equal probabilities would be a depolarizing channel
    t1 = 1.0 / -np.log1p(-a)                                            # p_r = a over time 1
    return _stack(thermal_relaxation_error(t1, (1.0 + b) * t1, 1.0, p1))    # t1 < t2 <= 2 t1


def kraus_op(q, ks):
    return ir.Op("kraus", qubits=(int(q),), table=np.asarray(ks, dtype=np.complex128))


def targets(W):
    return sorted({q for q in TARGETS + (W - 1,) if q < W})


def with_kraus(ops, W, rng, lo=0.05, hi=0.5):
    """``ops`` with Kraus records spliced in at random places behind the first layer: on every target qubit generic
    sets of m = 1, 2, 3, 4 operators and every constructor's channel"""
    ops = list(ops)
    head = next(i for i, o in enumerate(ops) if o.kind != "init") + W
    ts = targets(W)
    new = []
    for i, q in enumerate(ts):
        ms = (1, 2, 3, 4) if len(ts) <= 2 else ((1, 3), (2, 4))[i % 2]
        new += [kraus_op(q, isometry_kraus(rng, m)) for m in ms]
        whiches = (0, 1, 2, 3) if len(ts) <= 2 else ((0, 3), (1, 2))[i % 2]
        new += [kraus_op(q, constructor_kraus(rng, w, lo, hi)) for w in whiches]
    for op in new:
        ops.insert(int(rng.randint(head, len(ops) + 1)), op)
    return ops


def width_case(W):
    rng = np.random.RandomState(5000 + W)
    ops = with_kraus(nc.random_ops(W, 3000 + W, n_random=32, init=nc.WIDTH_INIT[W]), W, rng)
    rec, data = program.encode(ops)
    return dict(W=W, rec=rec, data=data, shots=nc.WIDTH_SHOTS[W], seed=8800 + W, meas=None, readout=None)


def realistic_case():
    """parameters of 1e-3: almost every draw takes the dominant operator, the others are rare"""
    W = 6
    rng = np.random.RandomState(61)
    ops = nc.random_ops(W, 6100, n_random=24)
    for i in range(40):
        w = i % 4
        ks = constructor_kraus(rng, w, 1e-3, 1e-3)
        ops.insert(int(rng.randint(W, len(ops) + 1)), kraus_op(int(rng.randint(W)), ks))
    rec, data = program.encode(ops)
    return dict(W=W, rec=rec, data=data, shots=2000, seed=6161, meas=None, readout=None)


def seed_case(seed, shots=1500):
    """one W = 4 program with Paulis, Kraus records, a permuted register and readout errors"""
    W = 4
    rng = np.random.RandomState(404)
    rec, data = program.encode(with_kraus(nc.random_ops(W, 444, n_random=24), W, rng))
    ro = np.array([[0.03, 0.05], [0.0, 0.2], [0.1, 0.0], [0.02, 0.02], [0.5, 0.5]])
    return dict(W=W, rec=rec, data=data, shots=shots, seed=seed, meas=[2, 0, 3, -1, 1], readout=ro)


def thermal_model():
    """thermal relaxation on every basis gate, composed with depolarizing errors, and a readout error: the shape of an
    Aer device model (T1 20 us, T2 30 us, gates of 200 ns and 1500 ns)"""
    one = thermal_relaxation_error(20e3, 30e3, 200.0)
    two = thermal_relaxation_error(20e3, 30e3, 1500.0)
    nm = NoiseModel()
    nm.add_all_qubit_quantum_error(one.compose(depolarizing_error(0.01, 1)), ["sx", "x", "id"])
    nm.add_all_qubit_quantum_error(two.expand(two).compose(depolarizing_error(0.05, 2)), ["cx"])
    nm.add_all_qubit_readout_error(ReadoutError([[0.97, 0.03], [0.05, 0.95]]))
    return nm


def lowered_case():
    return nc.lowered_case(1, nm=thermal_model())


def constructed_model():
    t = thermal_relaxation_error(20e3, 30e3, 2000.0, 0.05)
    nm = NoiseModel()
    nm.add_all_qubit_quantum_error(t.compose(depolarizing_error(0.02, 1)), "h")
    nm.add_all_qubit_quantum_error(pauli_error([("X", 0.01), ("Z", 0.02), ("I", 0.97)]).compose(t), "x")
    nm.add_all_qubit_readout_error(ReadoutError([[0.97, 0.03], [0.05, 0.95]]))
    return nm


def constructed_case():
    g = nc.models_05()
    qc = QCMRF(g["GRAPHS"][2], g["THETAS"]["2"][4], with_measurements=True)
    return nc.ingested_case(qc, constructed_model(), 78, most=600)


GPU_CASES = {"W=%d" % W: functools.partial(width_case, W) for W in WIDTHS}
GPU_CASES["realistic 1e-3"] = realistic_case
GPU_CASES.update({"seed %#x" % s: functools.partial(seed_case, s) for s in BIG_SEEDS})
GPU_CASES["prefix of 6000"] = functools.partial(seed_case, BIG_SEEDS[0], 6000)
GPU_CASES["lowered graph 1"] = lowered_case
GPU_CASES["constructed graph 2"] = constructed_case


@functools.lru_cache(maxsize=None)
def case(name):
    return GPU_CASES[name]()


@functools.lru_cache(maxsize=None)
def reference(name):
    """(words, alt_words, ambiguous, undetermined) of a named case: computed once, shared, left unchanged"""
    c = case(name)
    ref = exact_kraus_sample(c["rec"], c["data"], c["W"], c["shots"], c["seed"], c["meas"], c["readout"])
    for a in ref:
        a.setflags(write=False)
    return ref


def reference_of(c, **kw):
    return exact_kraus_sample(c["rec"], c["data"], c["W"], c["shots"], c["seed"], c["meas"], c["readout"], **kw)


# ---- forced channels: one outcome whatever is drawn ---------------------------------------------------------------------

_H = np.array([[1, 1], [1, -1]], dtype=np.complex128) / np.sqrt(2.0)


def forced_programs(W):
    """(label, (rec, data), expected basis index): full damping after X and a certain reset to |0> after H leave every
    qubit in |0>; a certain reset to |1> leaves it in |1>"""
    damp = _stack(amplitude_damping_error(1.0))
    r0, r1 = _stack(reset_error(1.0)), _stack(reset_error(0.0, 1.0))
    qs = targets(W)
    ones = sum(1 << q for q in qs)
    yield "X then damping 1", program.encode([ir.op_x(q) for q in qs] + [kraus_op(q, damp) for q in qs]), 0
    yield "H then reset to 0", program.encode([ir.op_u(q, _H) for q in range(W)] + [kraus_op(q, r0) for q in range(W)]), 0
    yield "reset to 1", program.encode([kraus_op(q, r1) for q in qs]), ones
    yield "H then reset to 1", program.encode([ir.op_u(q, _H) for q in range(W)] + [kraus_op(q, r1) for q in qs]
                                              + [kraus_op(q, r0) for q in range(W) if q not in qs]), ones


# ---- the effect the channels exist for: relaxation inflates the success rate ------------------------------------------------

def success_circuit():
    """the lowered circuit of one clique on two variables: W = 4, the clique's ancilla is classical bit 3"""
    qc = QCMRF([[0, 1]], [-0.4, -1.1, -0.2, -0.9], with_measurements=True)
    return transpile(qc, basis_gates=nc.BASIS), 2


def success_models(gamma=0.2):
    """amplitude damping gamma behind every sx, x, id and on both qubits of every cx, and its Pauli twirl (the nearest
    Pauli-only model: p_X = p_Y = gamma / 4, p_Z = (2 - gamma - 2 sqrt(1 - gamma)) / 4) in the same places"""
    damp = amplitude_damping_error(gamma)
    pz = (2.0 - gamma - 2.0 * np.sqrt(1.0 - gamma)) / 4.0
    twirl = pauli_error([("X", gamma / 4.0), ("Y", gamma / 4.0), ("Z", pz), ("I", 1.0 - gamma / 2.0 - pz)])
    out = []
    for e in (damp, twirl):
        nm = NoiseModel()
        nm.add_all_qubit_quantum_error(e, ["sx", "x", "id"])
        nm.add_all_qubit_quantum_error(e.tensor(e), ["cx"])
        out.append(nm)
    return out


def success_rate(dist_or_counts, n):
    """mass of the words whose bits above the n variable bits are all 0; takes a distribution over words or a counts
    dict of bit strings"""
    if isinstance(dist_or_counts, dict):
        tot = sum(dist_or_counts.values())
        return sum(v for k, v in dist_or_counts.items() if int(k.replace(" ", ""), 2) >> n == 0) / tot
    return float(dist_or_counts[:1 << n].sum())
