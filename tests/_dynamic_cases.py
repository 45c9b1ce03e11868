"""Streams and circuits of the tests of dynamic circuits (test infrastructure), shared by the host and the GPU tests.

``STREAMS`` names the record streams that test_gpu_noisy_dynamic.py holds to ``exact_dynamic_sample`` word by word, as builders
for a given width W: they use qubit 0, the middle qubit W // 2 and qubit W - 1, so that at every kernel shape the records
touch the lowest, a middle and the highest bit of the state index.  The host tests walk the same dictionary: the reference
alone stays within the ambiguity cap (the seeds are fixed, so that is a property of the cases), and every deliberately wrong
reference differs from the right one on some case.  ``CIRCUITS`` are the four circuits of the end-to-end tests."""
from __future__ import annotations

import functools

import numpy as np

from _dynamic_reference import exact_dynamic_sample
from qcmrf_amd import QCMRF, ir, program
from qcmrf_amd.circuit import Clbit, QuantumCircuit, Register
from qcmrf_amd.noise import NoiseModel, ReadoutError, depolarizing_error, pauli_error

SHOTS = 4096
SHAPES = ((3, False), (8, False), (11, False), (11, True))        # (W, slots): <64,1>, <64,8>, <256,1>, the slot kernel
CHAIN3 = [[0, 1], [1, 2]]
CHAIN3_THETA = [-0.4, -1.1, -0.2, -0.9, -0.3, -0.7, -0.5, -0.6]
FLIPS = (0.11, 0.23)


# ---- ops ---------------------------------------------------------------------------------------------------------------------

def ry(q, theta):
    return ir.op_u(q, ir.ry(theta), label="ry")


def cx(c, t):
    return ir.op_x(t, [c])


def measure(q, c, release=0, flips=FLIPS):
    return ir.Op("measure", target=q, mask=c, vals=(release,), table=flips)


def guard(span, mask, value, negate=0):
    return ir.Op("if", target=span, mask=mask, a=(value,), vals=(negate,))


def reset(q):
    return ir.Op("reset", target=q)


def pauli(q, px, pz, py):
    return ir.Op("pauli", qubits=(q,), table=np.array([1.0 - px - pz - py, px, pz, py]))      # index: x bit | z bit << 1


def damping(q, g):
    ks = np.array([[[1.0, 0.0], [0.0, np.sqrt(1.0 - g)]], [[0.0, np.sqrt(g)], [0.0, 0.0]]], dtype=np.complex128)
    return ir.Op("kraus", qubits=(q,), table=ks)


def damping2(q0, q1, g):
    k1 = np.zeros((4, 4), dtype=np.complex128)
    k1[0, 3] = np.sqrt(g)
    ks = np.array([np.diag([1.0, 1.0, 1.0, np.sqrt(1.0 - g)]).astype(np.complex128), k1])
    return ir.Op("kraus2", qubits=(q0, q1), table=ks)


# ---- streams -----------------------------------------------------------------------------------------------------------------
# classical bits 0, 1, 2: the final draw of qubits 0, W // 2 and W - 1 (with readout errors); bits 3 and up: MEASURE records

def _wires(W):
    return 0, W // 2, W - 1


def _prelude(W):
    a, m, z = _wires(W)
    return [ry(a, 1.1), ry(m, 0.7), ry(z, 2.0), cx(a, m)]


def s_reset(which, W):
    """RESET of a qubit in superposition, behind a cx that entangles it with another: the other's marginal must survive"""
    a, m, z = _wires(W)
    q = (a, m, z)[which]
    o = (m, z, a)[which]
    return [ry(q, 1.2), cx(q, o), ry(o, 0.4), reset(q), ry(q, 0.9), cx(o, q), measure(o, 3), ry(o, 0.3)]    # the MEASURE is draw 1 of stream 3


def s_if_bit(W):
    a, m, z = _wires(W)
    return _prelude(W) + [measure(a, 3), measure(m, 4), guard(1, 1 << 3, 1 << 3), ir.op_x(z), ry(m, 0.3)]     # bit 4: outside the mask


def s_if_value(W):
    a, m, z = _wires(W)
    return _prelude(W) + [measure(a, 3), measure(m, 4), measure(z, 5), guard(2, 0b111 << 3, 0b101 << 3), ir.op_x(m), ry(a, 0.8),
                          ry(z, 0.5)]


def s_if_bit63(W):
    a, m, z = _wires(W)
    return _prelude(W) + [measure(a, 63), guard(1, 1 << 63, 1 << 63), ir.op_x(z), ry(m, 0.3)]


def s_if_negate(W):
    a, m, z = _wires(W)
    return _prelude(W) + [measure(m, 3), guard(2, 1 << 3, 1 << 3, 1), ry(z, 0.6), ir.op_x(a), ry(m, 0.3)]


def s_span_kinds(W):
    """a span that holds a PAULI, a KRAUS, a KRAUS2 and a MEASURE record, and behind it a PAULI record whose draw index is 3
    where the span ran and 0 where it did not"""
    a, m, z = _wires(W)
    return _prelude(W) + [measure(a, 3), guard(4, 1 << 3, 1 << 3), pauli(m, 0.2, 0.1, 0.1), damping(m, 0.4), damping2(m, z, 0.5),
                          measure(z, 4), pauli(a, 0.3, 0.1, 0.2), ry(z, 0.4)]


def s_span_to_end(W):
    a, m, z = _wires(W)
    return _prelude(W) + [measure(a, 3), guard(2, 1 << 3, 0), ry(z, 0.9), pauli(m, 0.4, 0.0, 0.1)]


def s_two_ifs(W):
    a, m, z = _wires(W)
    return _prelude(W) + [measure(a, 3), guard(1, 1 << 3, 1 << 3), ir.op_x(m), guard(2, 1 << 3, 0), ry(z, 1.3), pauli(m, 0.3, 0.2, 0.0),
                          ry(a, 0.2)]


def s_never_written(W):
    a, m, z = _wires(W)
    return _prelude(W) + [measure(a, 3), guard(1, 1 << 5, 1 << 5), ir.op_x(z), guard(1, 1 << 5, 1 << 5, 1), ir.op_x(m), ry(a, 0.5)]


def s_rewrite(W):
    """a conditional MEASURE that rewrites the bit an earlier MEASURE wrote"""
    a, m, z = _wires(W)
    return _prelude(W) + [measure(a, 3), guard(1, 1 << 3, 1 << 3), measure(z, 3), ry(m, 0.3)]


STREAMS = {"reset bit 0": functools.partial(s_reset, 0), "reset middle": functools.partial(s_reset, 1),
           "reset top": functools.partial(s_reset, 2), "if one bit": s_if_bit, "if 3-bit value": s_if_value,
           "if bit 63": s_if_bit63, "if negate": s_if_negate, "span of every kind": s_span_kinds, "span to the end": s_span_to_end,
           "two ifs": s_two_ifs, "never written": s_never_written, "rewrite": s_rewrite}


@functools.lru_cache(maxsize=None)
def stream_case(name, W, shots=SHOTS):
    ops = STREAMS[name](W)
    n_meas = 64 if name == "if bit 63" else 6
    a, m, z = _wires(W)
    meas = [a, m, z] + [-1] * (n_meas - 3)
    if W == 3 and len({a, m, z}) < 3:
        raise AssertionError("the wires of a case must differ")
    rec, data = program.encode(ops, n_meas=n_meas)
    readout = np.zeros((n_meas, 2))
    readout[:3] = [[0.03, 0.05], [0.0, 0.2], [0.1, 0.0]]
    seed = 5000 + 17 * sorted(STREAMS).index(name) + W
    return dict(W=W, rec=rec, data=data, shots=shots, seed=seed, meas=meas, readout=readout)


def reference_of(c, **kw):
    return exact_dynamic_sample(c["rec"], c["data"], c["W"], c["shots"], c["seed"], c["meas"], c["readout"], **kw)


@functools.lru_cache(maxsize=None)
def reference(name, W):
    """(words, alt_words, ambiguous, undetermined) of a stream case: computed once, shared, left unchanged"""
    ref = reference_of(stream_case(name, W))
    for x in ref:
        x.setflags(write=False)
    return ref


def accept_stream(W):
    """a stream whose last writer of the fixed bit 3 stands inside a span"""
    a, m, z = _wires(W)
    return _prelude(W) + [measure(a, 3), measure(m, 4), guard(2, 1 << 4, 1 << 4), ry(z, 0.7), measure(z, 3), ry(m, 0.3), pauli(a, 0.2, 0.1, 0.1)]


# ---- circuits ----------------------------------------------------------------------------------------------------------------

def active_reset():
    """|+>, measured, flipped back if it read 1, measured again: under a readout error the second bit reads what the first
    misread"""
    qc = QuantumCircuit(1, 2, name="active_reset")
    qc.h(0)
    qc.measure(0, 0)
    qc.x(0).c_if(qc.clbits[0], 1)
    qc.measure(0, 1)
    return qc


def shared_ancilla_qcmrf(theta=CHAIN3_THETA, cliques=CHAIN3):
    """``QCMRF(chain(3), theta)`` as it is written for a device with qubit reuse: every clique ancilla on ONE qubit, a ``reset``
    behind each ancilla measurement; the classical bits are those of the original"""
    src = QCMRF(cliques, theta, with_measurements=True)
    n = src.num_vertices
    qc = QuantumCircuit(n + 2, src.num_clbits, name="shared_ancilla")
    for ci in src.data:
        qs = [min(src.find_bit(q).index, n + 1) for q in ci.qubits]
        cs = [src.find_bit(c).index for c in ci.clbits]
        qc.append(ci.operation, qs, cs)
        if ci.operation.name == "measure" and qs[0] == n + 1:
            qc.reset(n + 1)
    return qc, src


def register_condition():
    """three qubits measured into a register, a gate conditioned on the register's integer value"""
    qc = QuantumCircuit(4, 4, name="register_condition")
    for q, th in enumerate((1.0, 1.4, 0.6)):
        qc.ry(th, q)
    qc.measure([0, 1, 2], [0, 1, 2])
    three = Register(3, "low", Clbit)
    three._bits = qc.clbits[:3]                                # a register over the three low bits of the circuit
    qc.x(3).c_if(three, 5)
    qc.ry(0.4, 0)
    qc.measure(3, 3)
    return qc


def if_else_circuit():
    qc = QuantumCircuit(2, 2, name="if_else")
    qc.ry(1.2, 0)
    qc.measure(0, 0)
    with qc.if_test((qc.clbits[0], 1)) as else_:
        qc.x(1)
        qc.h(0)
    with else_:
        qc.ry(0.8, 1)
    qc.measure(1, 1)
    return qc


CIRCUITS = {"active reset": active_reset, "shared ancilla": lambda: shared_ancilla_qcmrf()[0],
            "register condition": register_condition, "if else": if_else_circuit}


def reset_only_circuit():
    """resets and no condition: what method='density_matrix' runs exactly"""
    qc = QuantumCircuit(2, 3, name="reset_only")
    qc.ry(1.1, 0)
    qc.cx(0, 1)
    qc.reset(0)
    qc.ry(0.7, 0)
    qc.cx(0, 1)
    qc.reset(1)
    qc.h(1)
    qc.measure([0, 1], [0, 2])
    return qc


def readout_model(f0=FLIPS[0], f1=FLIPS[1], gate_error=0.02):
    nm = NoiseModel()
    if gate_error:
        nm.add_all_qubit_quantum_error(depolarizing_error(gate_error, 1), ["x", "h", "ry"])
    nm.add_all_qubit_readout_error(ReadoutError([[1.0 - f0, f0], [f1, 1.0 - f1]]))
    return nm


def x_error_model(p=0.25):
    """an X error behind every x gate and nothing else: it can occur only where the gate does"""
    nm = NoiseModel()
    nm.add_all_qubit_quantum_error(pauli_error([("X", p), ("I", 1.0 - p)]), ["x"])
    return nm
