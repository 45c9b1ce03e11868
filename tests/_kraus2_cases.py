"""Programs of the tests of two-qubit Kraus records (test infrastructure), shared by the host and the GPU tests.
``GPU_CASES`` names every case that test_gpu_kraus2_exact.py runs through ``check_kraus_words``; the host tests walk the same
dictionary to assert that the reference alone stays within the ambiguity cap (the seeds are fixed, so that is a property of
the cases) and to run the comparison against deliberately wrong references."""
from __future__ import annotations

import functools

import numpy as np

import _kraus_cases as kc
import _noise_exact_cases as nc
from _kraus2_reference import exact_kraus2_sample, kraus2_density_distribution
from qcmrf_amd import QCMRF, ir, program
from qcmrf_amd.backend import QsvBackend
from qcmrf_amd.noise import (NoiseModel, ReadoutError, coherent_unitary_error, depolarizing_error, mixed_unitary_error,
                             pauli_error)
from qcmrf_amd.run_experiment import cx_over_rotation
from qcmrf_amd.transpile import transpile

# each qubit of a pair below, at and above the lane boundary (bit 5) and the wave boundary (bits 6 and 7) of every kernel
# instantiation; both sides of the 7 / 8 and 10 / 11 switches between them
WIDTHS = (2, 3, 7, 8, 10, 11, 13)
SHOTS = {2: 2000, 3: 2000, 7: 2000, 8: 1500, 10: 1000, 11: 500, 13: 200}
PAIRS = ((0, 1), (1, 0), (0, 5), (5, 6), (6, 5), (7, 8), (0, -1), (-2, -1))       # negative: counted from W
BIG_SEED = 2 ** 32 + 7
CHAIN3 = [[0, 1], [1, 2]]
CHAIN3_THETA = [-0.4, -1.1, -0.2, -0.9, -0.3, -0.7, -0.5, -0.6]


def pairs(W):
    """the ordered pairs of PAIRS that fit into W qubits, each once"""
    out = []
    for a, b in PAIRS:
        a, b = (a + W if a < 0 else a), (b + W if b < 0 else b)
        if 0 <= a < W and 0 <= b < W and a != b and (a, b) not in out:
            out.append((a, b))
    return out


# ---- channels -------------------------------------------------------------------------------------------------------------

def isometry_kraus2(rng, m):
    """m generic two-qubit Kraus operators: the 4 x 4 blocks of a random 4m x 4 isometry (sum K^dg K = 1)"""
    q, _ = np.linalg.qr(rng.randn(4 * m, 4) + 1j * rng.randn(4 * m, 4))
    return q.reshape(m, 4, 4)


def unitary4(rng):
    return isometry_kraus2(rng, 1)[0]


def correlated_damping(g):
    """|11> decays to |00> with probability g: K_0 = diag(1, 1, 1, sqrt(1 - g)), K_1 = sqrt(g) |00><11|"""
    k1 = np.zeros((4, 4), dtype=np.complex128)
    k1[0, 3] = np.sqrt(g)
    return np.array([np.diag([1.0, 1.0, 1.0, np.sqrt(1.0 - g)]).astype(np.complex128), k1])


def _stack(err):
    (kind, _, ks), = err.terms()
    assert kind == "kraus2"
    return ks


def menu(rng):
    """the stacks a width case cycles through: generic sets of m = 1, 2, 4 and 16, a coherent ZX rotation, a mixed-unitary
    set, a correlated damping set and one channel with a parameter of 1e-3"""
    zx = cx_over_rotation(0.3)
    mixed = mixed_unitary_error([(np.eye(4), 0.7), (unitary4(rng), 0.2), (zx, 0.1)])
    return [isometry_kraus2(rng, 1), isometry_kraus2(rng, 2), isometry_kraus2(rng, 4), isometry_kraus2(rng, 16),
            _stack(coherent_unitary_error(zx)), _stack(mixed), correlated_damping(rng.uniform(0.2, 0.6)), correlated_damping(1e-3)]


def kraus2_op(q0, q1, ks):
    return ir.Op("kraus2", qubits=(int(q0), int(q1)), table=np.asarray(ks, dtype=np.complex128))


def with_kraus2(ops, W, rng):
    """``ops`` with KRAUS2 records spliced in at random places behind the first layer: every stack of the menu, every pair
    of ``pairs(W)``"""
    ops = list(ops)
    head = next(i for i, o in enumerate(ops) if o.kind != "init") + W
    ps, stacks = pairs(W), menu(rng)
    for i in range(max(len(ps), len(stacks))):
        ops.insert(int(rng.randint(head, len(ops) + 1)), kraus2_op(*ps[i % len(ps)], stacks[i % len(stacks)]))
    return ops


def random_ops(W, seed, n_random):
    """a seeded random program of every unitary kind, PAULI, KRAUS and KRAUS2 records"""
    rng = np.random.RandomState(seed)
    ops = nc.random_ops(W, seed + 1, n_random=n_random, init=("uniform", None, "mid")[W % 3])
    return with_kraus2(kc.with_kraus(ops, W, rng), W, rng)


def width_case(W):
    rec, data = program.encode(random_ops(W, 7000 + W, 24 if W < 13 else 12))
    return dict(W=W, rec=rec, data=data, shots=SHOTS[W], seed=9900 + W, meas=None, readout=None)


def seed_case(seed, shots=1500):
    """one W = 4 program with every record kind, a permuted register and readout errors"""
    rec, data = program.encode(random_ops(4, 414, 24))
    ro = np.array([[0.03, 0.05], [0.0, 0.2], [0.1, 0.0], [0.02, 0.02], [0.5, 0.5]])
    return dict(W=4, rec=rec, data=data, shots=shots, seed=seed, meas=[2, 0, 3, -1, 1], readout=ro)


def slot_case(W):
    """the slot path past the LDS widths: few records, few shots (the numpy reference evolves 2^W x shots amplitudes)"""
    rng = np.random.RandomState(1400 + W)
    ops = with_kraus2(nc.random_ops(W, 1500 + W, n_random=8), W, rng)
    rec, data = program.encode(ops)
    return dict(W=W, rec=rec, data=data, shots=96, seed=1600 + W, meas=None, readout=None)


# ---- through the host path: a chain of 3 variables under depolarizing + coherent two-qubit + readout errors -------------------

def chain3(lowered):
    qc = QCMRF(CHAIN3, CHAIN3_THETA, with_measurements=True)
    return transpile(qc, basis_gates=nc.BASIS) if lowered else qc


def lowered_model(eps=0.2):
    nm = NoiseModel()
    nm.add_all_qubit_quantum_error(depolarizing_error(0.01, 1), ["sx", "x"])
    nm.add_all_qubit_quantum_error(depolarizing_error(0.02, 2).compose(coherent_unitary_error(cx_over_rotation(eps))), ["cx"])
    nm.add_all_qubit_readout_error(ReadoutError([[0.97, 0.03], [0.05, 0.95]]))
    return nm


def constructed_model(eps=0.2):
    """the same on the gate names a constructed circuit carries: its two-qubit gate is ``cp``"""
    nm = NoiseModel()
    nm.add_all_qubit_quantum_error(depolarizing_error(0.02, 1), ["h", "x"])
    nm.add_all_qubit_quantum_error(coherent_unitary_error(cx_over_rotation(eps)), ["cp"])
    nm.add_all_qubit_readout_error(ReadoutError([[0.97, 0.03], [0.05, 0.95]]))
    return nm


def run_case(lowered, measure, seed, shots=600):
    """a circuit under a noise model as ``run(noisy_measure=measure)`` hands it to the engine"""
    qc, nm = chain3(lowered), (lowered_model() if lowered else constructed_model())
    ing, rec, data, clist, meas, readout, _, state, (mode, width, n_measure) = QsvBackend._prepare_noisy(qc, nm, "lds", measure)
    assert mode == measure and ing.n_kraus2 > 0
    return dict(W=width, rec=rec, data=data, shots=shots, seed=seed, meas=meas, readout=readout, n_measure=n_measure)


GPU_CASES = {"W=%d" % W: functools.partial(width_case, W) for W in WIDTHS}
GPU_CASES["seed"] = functools.partial(seed_case, BIG_SEED)
GPU_CASES["prefix of 2000"] = functools.partial(seed_case, BIG_SEED, 2000)
GPU_CASES.update({"slots W=%d" % W: functools.partial(slot_case, W) for W in (11, 14)})
for _low in (True, False):
    for _m in ("deferred", "in_place"):
        GPU_CASES["%s chain(3) %s" % ("lowered" if _low else "constructed", _m)] = functools.partial(run_case, _low, _m, 300 + 7 * _low)


@functools.lru_cache(maxsize=None)
def case(name):
    return GPU_CASES[name]()


def reference_of(c, **kw):
    return exact_kraus2_sample(c["rec"], c["data"], c["W"], c["shots"], c["seed"], c["meas"], c["readout"], **kw)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(words, alt_words, ambiguous, undetermined) of a named case: computed once, shared, left unchanged"""
    ref = reference_of(case(name))
    for a in ref:
        a.setflags(write=False)
    return ref


# ---- forced channels: one outcome whatever is drawn -------------------------------------------------------------------------

def forced_programs(W):
    """(label, (rec, data), expected basis index).  X on a, then a swap-like unitary (i SWAP: |01> <-> |10> with a phase)
    as a KRAUS2 record of one operator on (a, b): the excitation moves to b.  X on both, then full correlated damping:
    |11> ends in |00>, whichever operator the draw would prefer."""
    iswap = np.array([[1, 0, 0, 0], [0, 0, 1j, 0], [0, 1j, 0, 0], [0, 0, 0, 1]], dtype=np.complex128)
    for a, b in pairs(W):
        yield "X(%d) then iSWAP(%d, %d)" % (a, a, b), program.encode([ir.op_x(a), kraus2_op(a, b, [iswap])]), 1 << b
        yield ("X(%d) X(%d) then full damping" % (a, b),
               program.encode([ir.op_x(a), ir.op_x(b), kraus2_op(a, b, correlated_damping(1.0))]), 0)


# ---- the effect the record exists for: a coherent error is not its Pauli twirl ----------------------------------------------

def coherent_and_twirl(eps=0.35):
    """the ZX over-rotation exp(-i eps/2 Z(x)X) behind every cx and its Pauli twirl, the Pauli error of the same process
    fidelity: ZX (label 'XZ': the rightmost character acts on error qubit 0) with probability sin^2(eps / 2)"""
    p = np.sin(0.5 * eps) ** 2
    out = []
    for e in (coherent_unitary_error(cx_over_rotation(eps)), pauli_error([("XZ", p), ("II", 1.0 - p)])):
        nm = NoiseModel()
        nm.add_all_qubit_quantum_error(e, ["cx"])
        out.append(nm)
    return out


def exact_distribution(qc, nm):
    """the numpy walker's distribution over the recorded words of ``qc`` under ``nm`` (None: ideal)"""
    from qcmrf_amd import ingest as ing_mod
    ing = ing_mod.ingest(qc, noise=nm)
    rec, data = program.encode(ing.ops)
    meas = [ing.measure.get(c, -1) for c in range(ing.num_clbits)]
    ro = [ing.readout.get(c, (0.0, 0.0)) for c in range(ing.num_clbits)] if ing.readout else None
    return kraus2_density_distribution(rec, data, ing.num_qubits, meas, ro)


def post_selected(dist, n):
    """(the distribution of the n variable bits given that every bit above them is 0, the mass of that event)"""
    rate = float(dist[:1 << n].sum())
    return dist[:1 << n] / rate, rate


@functools.lru_cache(maxsize=None)
def effect_expected():
    """{name: (post-selected distribution, all-ancillas-zero rate)} for the ideal circuit, the coherent error and its
    twirl on the lowered chain of 3 variables, from the numpy walker"""
    T = chain3(True)
    coh, twirl = coherent_and_twirl()
    return {name: post_selected(exact_distribution(T, nm), 3) for name, nm in (("ideal", None), ("coherent", coh), ("twirl", twirl))}
