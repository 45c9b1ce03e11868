"""Programs and the comparison helper of the word-by-word noisy-shot tests (test infrastructure).

``check_words`` is the one assertion every case goes through; the builders give the programs.  They live here, not in
test_gpu_noise_exact.py, so that the host tests can run the same cases against a deliberately wrong reference and
show that the helper notices (test_noise_reference.py)."""
from __future__ import annotations

import json
import os

import numpy as np

from qcmrf_amd import QCMRF, ingest as ing_mod, ir, program
from qcmrf_amd.noise import NoiseModel, ReadoutError, depolarizing_error, pauli_error
from qcmrf_amd.transpile import transpile

BASIS = ["cx", "id", "rz", "sx", "x"]
WIDTHS = (1, 2, 3, 5, 6, 7, 10, 11, 12, 13)
# per width: how the program starts ("uniform": INIT_UNIFORM of a partial mask first, "mid": INIT_UNIFORM in
# mid-program, "zero": INIT_ZERO first, None: no init record at all) and its shots: 2^W x shots x records stays below
# 2e8, far inside the 5e9 a case may cost
WIDTH_INIT = {1: "zero", 2: None, 3: "uniform", 5: None, 6: "mid", 7: "uniform", 10: "zero", 11: "uniform", 12: "mid", 13: None}
WIDTH_SHOTS = {1: 2000, 2: 2000, 3: 2000, 5: 2000, 6: 2000, 7: 2000, 10: 1000, 11: 500, 12: 300, 13: 200}
SEEDS = (0, 2 ** 32 - 1, 2 ** 32, 2 ** 63 + 12345, 2 ** 64 - 1)

TALLY = {}       # family -> [shots compared, ambiguous shots, mismatches]: what the pull request text reports


def ambiguity_cap(shots):
    return max(2, shots // 1000)


def check_words(got, words, alt_words, ambiguous, family, label=""):
    """every word of a call against the reference: equal where the reference is sure, one of the two candidates where
    the final draw is within rounding distance of a boundary, and few such shots"""
    got = np.asarray(got, dtype=np.uint64)
    assert got.shape == words.shape, "%s %s: %d words for %d shots" % (family, label, got.size, words.size)
    n_amb = int(ambiguous.sum())
    bad = np.flatnonzero((got != words) & ~(ambiguous & (got == alt_words)))
    t = TALLY.setdefault(family, [0, 0, 0])
    t[0] += got.size
    t[1] += n_amb
    t[2] += bad.size
    print("EXACT family=%s case=%s shots=%d ambiguous=%d mismatches=%d" % (family, label, got.size, n_amb, bad.size))
    assert n_amb <= ambiguity_cap(got.size), "%s %s: %d ambiguous shots of %d" % (family, label, n_amb, got.size)
    assert bad.size == 0, "%s %s: %d of %d shots differ, first at shot %d: got %#x, reference %#x%s" % (
        family, label, bad.size, got.size, bad[0], int(got[bad[0]]), int(words[bad[0]]),
        " or %#x" % int(alt_words[bad[0]]) if ambiguous[bad[0]] else "")


# ---- seeded random programs ----------------------------------------------------------------------------------------

def _unitary(rng):
    q, r = np.linalg.qr(rng.randn(2, 2) + 1j * rng.randn(2, 2))
    return q * (np.diag(r) / np.abs(np.diag(r)))


def _controls(rng, W, taken, most=4):
    free = [q for q in range(W) if q not in taken]
    n = rng.randint(0, min(most, len(free)) + 1)
    ctrls = [int(c) for c in rng.permutation(free)[:n]]
    return ctrls, [int(v) for v in rng.randint(0, 2, n)]


def _pauli(rng, qubits):
    return ir.Op("pauli", qubits=tuple(int(q) for q in qubits), table=rng.dirichlet(np.ones(4 ** len(qubits))))


def random_ops(W, seed, n_random=48, init=None):
    """roughly 40-80 records: controlled 2x2 and MCX with 0-4 controls of random polarity, DIAG on 1..min(W, 8) qubits in
    random order, MCPHASE with mixed polarities, 1- and 2-qubit Pauli records with generic probabilities; every kind also
    on qubit 0 and on qubit W - 1, 2-qubit Paulis with q0 < q1 and q0 > q1"""
    rng = np.random.RandomState(seed)
    ops = []
    if init == "uniform":
        ops.append(ir.op_init(int(rng.randint(1, max(2, (1 << W) - 1)))))
    elif init == "zero":
        ops.append(ir.op_init(0))
    ops += [ir.op_u(q, _unitary(rng)) for q in range(W)]           # mass everywhere, so that controls fire
    kinds = ["u", "x", "diag", "mcphase", "pauli1"] + (["pauli2"] if W >= 2 else [])

    def one(kind, q):
        if kind in ("u", "x"):
            ctrls, vals = _controls(rng, W, (q,))
            return ir.op_u(q, _unitary(rng), ctrls, vals) if kind == "u" else ir.op_x(q, ctrls, vals)
        if kind == "diag":
            k = rng.randint(1, min(W, 8) + 1)
            qs = [q] + [int(x) for x in rng.permutation([x for x in range(W) if x != q])[:k - 1]]
            return ir.op_diag(rng.permutation(qs), np.exp(2j * np.pi * rng.rand(1 << k)))
        if kind == "mcphase":
            ctrls, vals = _controls(rng, W, (q,), most=3)
            return ir.op_mcphase([q] + ctrls, float(rng.uniform(-np.pi, np.pi)), [int(rng.randint(0, 2))] + vals)
        if kind == "pauli1":
            return _pauli(rng, [q])
        other = int(rng.choice([x for x in range(W) if x != q]))
        return _pauli(rng, [q, other])

    for i in range(n_random):
        if init == "mid" and i == n_random // 2:
            ops.append(ir.op_init(int(rng.randint(1, (1 << W) - 1))))
            ops += [ir.op_u(q, _unitary(rng), *_controls(rng, W, (q,), most=1)) for q in range(W)]
        ops.append(one(kinds[rng.randint(len(kinds))], int(rng.randint(W))))
    for kind in kinds:                                             # both ends of the register, every kind
        for q in sorted({0, W - 1}):
            ops.append(one(kind, q))
    if W >= 2:
        ops += [_pauli(rng, [0, W - 1]), ir.op_u(0, _unitary(rng), [W - 1], [0]), _pauli(rng, [W - 1, 0])]
    return ops


def width_case(W):
    rec, data = program.encode(random_ops(W, 1000 + W, init=WIDTH_INIT[W]))
    return dict(W=W, rec=rec, data=data, shots=WIDTH_SHOTS[W], seed=7700 + W, meas=None, readout=None)


# ---- forced Paulis: probability 1 on one index, so no random number decides anything ------------------------------------

_H = np.array([[1, 1], [1, -1]], dtype=np.complex128) / np.sqrt(2.0)


def forced_pauli_programs(W, qubits, p):
    """(|0..0> -> P, x mask) and (H^W -> P -> H^W, z mask) for the Pauli with index p on ``qubits``: both programs end
    in that one basis state (H X H = Z, H Z H = X)"""
    table = np.zeros(4 ** len(qubits))
    table[p] = 1.0
    P = ir.Op("pauli", qubits=tuple(qubits), table=table)
    x = z = 0
    for j, q in enumerate(qubits):
        x |= ((p >> (2 * j)) & 1) << q
        z |= ((p >> (2 * j + 1)) & 1) << q
    hs = [ir.op_u(q, _H) for q in range(W)]
    return (program.encode([P]), x), (program.encode(hs + [P] + hs), z)


def forced_pauli_cases(W):
    """all 3 one-qubit and all 15 two-qubit non-identity indices; pairs in both orders, adjacent and not"""
    singles = sorted({0, W // 2, W - 1})
    pairs = [(0, 1), (1, 0), (0, W - 1), (W - 1, 0), (1, W - 2), (W - 2, 1)] if W >= 4 else [(0, 1), (1, 0)]
    for q in singles:
        for p in range(1, 4):
            yield (q,), p
    for qs in pairs:
        for p in range(1, 16):
            yield qs, p


# ---- through the host path -----------------------------------------------------------------------------------------------

def models_05():
    return json.load(open(os.path.join(os.path.dirname(__file__), "golden", "models_0.5.json")))


def reference_model(readout=True):
    nm = NoiseModel()
    nm.add_all_qubit_quantum_error(depolarizing_error(0.01, 1), ["sx", "x"])
    nm.add_all_qubit_quantum_error(depolarizing_error(0.05, 2), ["cx"])
    if readout:
        nm.add_all_qubit_readout_error(ReadoutError([[0.97, 0.03], [0.05, 0.95]]))
    return nm


def ingested_case(qc, nm, seed, budget=4e8, most=2000):
    """a circuit under a noise model as the backend hands it to the engine; shots sized so that 2^W x shots x records
    stays near ``budget``"""
    ing = ing_mod.ingest(qc, noise=nm)
    rec, data = program.encode(ing.ops)
    meas = [ing.measure.get(c, -1) for c in range(ing.num_clbits)]
    ro = np.array([ing.readout.get(c, (0.0, 0.0)) for c in range(ing.num_clbits)]) if ing.readout else None
    shots = int(min(most, max(100, budget // ((1 << ing.num_qubits) * max(1, len(rec))))))
    return dict(W=ing.num_qubits, rec=rec, data=data, shots=shots, seed=seed, meas=meas, readout=ro)


def lowered_case(j, nm=None, **kw):
    g = models_05()
    T = transpile(QCMRF(g["GRAPHS"][j], g["THETAS"][str(j)][1], with_measurements=True), basis_gates=BASIS)
    return ingested_case(T, reference_model() if nm is None else nm, 4242 + j, **kw)


def constructed_case(**kw):
    g = models_05()
    qc = QCMRF(g["GRAPHS"][2], g["THETAS"]["2"][4], with_measurements=True)
    nm = NoiseModel()
    nm.add_all_qubit_quantum_error(depolarizing_error(0.02, 1), "h")
    nm.add_all_qubit_quantum_error(pauli_error([("X", 0.01), ("Z", 0.02), ("I", 0.97)]), "x")
    return ingested_case(qc, nm, 77, **kw)


# ---- measurement mapping, seeds, identity-heavy streams --------------------------------------------------------------------

def mapping_case(n_meas=64, seed=31):
    """W = 5: more classical bits than qubits, -1 entries, repeated qubits, readout probabilities that include exact
    0.0 and 1.0, and certain flips on bits that no measurement writes (they must stay 0)"""
    W = 5
    rng = np.random.RandomState(seed)
    rec, data = program.encode(random_ops(W, 555, n_random=30))
    meas = [int(q) for q in rng.randint(-1, W, n_meas)]
    head = [W - 1, -1, 0, 0][:n_meas]
    meas[:len(head)] = head
    if n_meas == 64:
        meas[62:] = [-1, 2]                                        # bit 63 measured, bit 62 not
    ro = rng.uniform(0.0, 0.3, (n_meas, 2))
    ro[rng.rand(n_meas, 2) < 0.15] = 0.0
    ro[rng.rand(n_meas, 2) < 0.15] = 1.0
    ro[[j for j, q in enumerate(meas) if q < 0]] = 1.0             # a flip that must not happen
    return dict(W=W, rec=rec, data=data, shots=2000, seed=90210, meas=meas, readout=ro)


def seed_case(seed):
    """one W = 4 program with Paulis, a permuted register and readout errors, for the seeds of SEEDS"""
    W = 4
    rec, data = program.encode(random_ops(W, 444, n_random=24))
    ro = np.array([[0.03, 0.05], [0.0, 0.2], [0.1, 0.0], [0.02, 0.02], [0.5, 0.5]])
    return dict(W=W, rec=rec, data=data, shots=1500, seed=seed, meas=[2, 0, 3, -1, 1], readout=ro)


def identity_heavy_case():
    """Pauli records that draw the identity 999 times in 1000, interleaved with records that never do: a draw counter
    that does not advance on an identity shifts every later draw"""
    W = 4
    rng = np.random.RandomState(99)
    ops = [ir.op_u(q, _unitary(rng)) for q in range(W)]
    for i in range(24):
        q = int(rng.randint(W))
        rare = np.concatenate([[0.999], 0.001 * rng.dirichlet(np.ones(3))])
        ops.append(ir.Op("pauli", qubits=(q,), table=rare))
        t = int(rng.randint(W))
        ops.append(ir.op_u(t, _unitary(rng), *_controls(rng, W, (t,), most=2)))
        never = rng.dirichlet(np.ones(15 if i % 2 else 3))
        qs = (q, int((q + 1 + rng.randint(W - 1)) % W)) if i % 2 else (int(rng.randint(W)),)
        ops.append(ir.Op("pauli", qubits=qs, table=np.concatenate([[0.0], never])))
    rec, data = program.encode(ops)
    return dict(W=W, rec=rec, data=data, shots=2000, seed=2 ** 40 + 5, meas=None, readout=None)


def reference_of(case, **kw):
    from _philox_reference import exact_noisy_sample
    return exact_noisy_sample(case["rec"], case["data"], case["W"], case["shots"], case["seed"], case["meas"], case["readout"], **kw)
