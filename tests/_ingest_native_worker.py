"""TEST INFRASTRUCTURE: the native block reader on circuits built with the strict Qiskit double (tests/strict_qiskit), in
a child process with the double FIRST on sys.path so that qcmrf_amd takes its "Qiskit is importable" branch (as
tests/_strict_worker.py does).  There ``circuit.data`` is a view object, ``qubits`` a fresh list per read, names and
definitions are properties, bits compare equal across registers of one name, and AND nests as Qiskit nests it.

    python tests/_ingest_native_worker.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE, os.path.join(HERE, "strict_qiskit")):
    if p in sys.path:
        sys.path.remove(p)
    sys.path.insert(0, p)

import qiskit                                        # noqa: E402
assert "strict-double" in qiskit.__version__, qiskit.__file__
from qiskit import QuantumCircuit                    # noqa: E402
from qiskit.circuit import CircuitInstruction, QuantumRegister   # noqa: E402
from qiskit.circuit.library import AND               # noqa: E402
import qcmrf_amd                                     # noqa: E402
from qcmrf_amd import QCMRF, workloads               # noqa: E402
from qcmrf_amd import ingest as ing_mod              # noqa: E402

from _ingest_compare import assert_keys_equal, assert_same, blocks_of, both   # noqa: E402

assert qcmrf_amd.HAVE_QISKIT is True
assert ing_mod.native_available(), "qcmrf_amd._ingest_native is not built (python -m qcmrf_amd.build)"


def theta(cliques):
    return workloads.theta_halfnorm(workloads.dimension(cliques))


def agree(qc, n_blocks, path="native"):
    a, b = both(qc)
    assert a.ingest_path == path, a.ingest_path
    assert sum(o.kind == "diag" and len(o.qubits) > 1 for o in a.ops) == n_blocks
    assert_same(a, b)
    return a


# 1. the circuits of the reference's constructor, on the double
g = json.load(open(os.path.join(HERE, "golden", "config1.json")))
for cliques, th in (([[0, 1]], theta([[0, 1]])), ([[0, 1, 2]], theta([[0, 1, 2]])), (g["cliques"], g["theta"]),
                    (workloads.chain(4), theta(workloads.chain(4)))):
    qc = QCMRF(cliques, th)
    assert assert_keys_equal(qc) == 2 * len(cliques)
    agree(qc, 2 * len(cliques))


# 2. a block built by hand, its ANDs wrapped ``wrap`` more times by append(circuit)
def hand_block(k, lams, wrap):
    blk = QuantumCircuit(k + 2, name="cU_C0")
    for y, lam in enumerate(lams):
        flags = [1 if (y >> i) & 1 else -1 for i in range(k)]
        for part in range(3):
            if part == 1:
                blk.cp(lam, k, k + 1)
                continue
            a = AND(k, flags)
            for _ in range(wrap):
                outer = QuantumCircuit(k + 1, name="and")
                outer.append(a, list(range(k + 1)))
                a = outer
            blk.append(a, list(range(k + 1)))
    n = k + 2
    qc = QuantumCircuit(n, n, name="hand")
    for i in range(n):
        qc.h(i)
    qc.append(blk, list(range(n)))
    for i in range(n):
        qc.measure(i, i)
    return qc


lams = [0.1, -0.2, 0.3, -0.4]
plain, wrapped = hand_block(2, lams, 0), hand_block(2, lams, 1)
for qc in (plain, wrapped, hand_block(2, lams, 3)):
    assert assert_keys_equal(qc) == 1
d0, d1 = blocks_of(plain)[0], blocks_of(wrapped)[0]
assert len(d1.data[0].operation.definition.data[0].operation.definition.data) == 1      # one wrapper more than Qiskit's own
assert ing_mod._ingest_native.read_block(d0)[0] == ing_mod._ingest_native.read_block(d1)[0]  # unwrapped to the same signature
assert_same(agree(plain, 1), agree(wrapped, 1))
# ... past the eight levels that are followed: whatever the Python code makes of it, the native path makes the same
deep = hand_block(2, lams, 9)
a, b = both(deep)
assert_same(a, b)


# 3. operations without a ``.condition`` attribute at all
def strip_conditions(circuit, depth=0):
    for ci in circuit.data:
        op = ci.operation
        op.__dict__.pop("condition", None)
        assert not hasattr(op, "condition")
        if op.name not in ing_mod._PRIMITIVES and op.name not in ("measure", "barrier") and depth < 6:
            strip_conditions(op.definition, depth + 1)


qc = QCMRF([[0, 1, 2]], theta([[0, 1, 2]]))
strip_conditions(qc)
assert assert_keys_equal(qc) == 2
agree(qc, 2)

# 4. bits equal to, but not, the definition's own: the Python code finds them by equality, the reader leaves them to it
qc = QCMRF([[0, 1, 2]], theta([[0, 1, 2]]))
d = blocks_of(qc)[0]
twin = QuantumRegister(len(d.qubits), d.qregs[0].name)
ci = d._data[1]
other = tuple(twin[d.find_bit(q).index] for q in ci.qubits)
assert all(x == y and x is not y for x, y in zip(other, ci.qubits))
d._data[1] = CircuitInstruction(ci.operation, other, ())
assert ing_mod._ingest_native.read_block(d) is None and ing_mod._read_block(d) is not None
agree(qc, 2, path="mixed")
# ... one level down, in an AND
qc = QCMRF([[0, 1, 2]], theta([[0, 1, 2]]))
d = blocks_of(qc)[0]
inner = d.data[0].operation.definition
twin = QuantumRegister(len(inner.qubits), inner.qregs[0].name) if len(inner.qregs) == 1 else None
if twin is not None:
    ci = inner._data[0]
    inner._data[0] = CircuitInstruction(ci.operation, tuple(twin[inner.find_bit(q).index] for q in ci.qubits), ())
    assert ing_mod._ingest_native.read_block(d) is None and ing_mod._read_block(d) is not None
    agree(qc, 2, path="mixed")

print("ingest-native strict worker ok")
