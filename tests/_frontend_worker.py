"""TEST INFRASTRUCTURE: the native front end on circuits built with the strict Qiskit double (tests/strict_qiskit), in a
child process with the double FIRST on sys.path so that qcmrf_amd takes its "Qiskit is importable" branch (as
tests/_ingest_native_worker.py does).  There ``circuit.data`` is a view object, ``qubits`` and ``clbits`` are fresh lists
per read, and bits compare equal across registers of one name.

    python tests/_frontend_worker.py
"""
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
from qiskit.circuit import CircuitInstruction, QuantumRegister   # noqa: E402
import qcmrf_amd                                     # noqa: E402
from qcmrf_amd import ingest as ing_mod              # noqa: E402

import _frontend_cases as fc                         # noqa: E402

assert qcmrf_amd.HAVE_QISKIT is True
assert ing_mod.native_available(), "qcmrf_amd._ingest_native is not built (python -m qcmrf_amd.build)"

# 1. the circuits of the reference's constructor, on the double: taken, and equal to the pipeline
for name in sorted(fc.ACCEPTED):
    if name in ("baseline2", "baseline4"):
        continue                                     # (the in-tree run has them; the double builds them slowly)
    for seed in fc.SEEDS[:2]:
        fc.assert_accepted_and_equal(fc.accepted(name, seed))
qc = fc.accepted("chain9")
on, off = fc.program_bytes(qc, True), fc.program_bytes(qc, False)
assert on[0] == "blocks" and off[0] == "passes" and on[1:] == off[1:]

# 2. off the grammar: declined, or what the pipeline answers
for spoil in fc.SPOILS:
    how = fc.declined_or_equal(fc.spoiled(spoil))
    assert how in ("declined", "equal") or how.startswith("ValueError"), (spoil, how)
    assert how != "equal" or spoil == "wire_never_opened", (spoil, how)
assert fc.declined_or_equal(fc.spoiled(None)) == "equal"

# 3. bits equal to, but not, the circuit's own: the pipeline finds them by equality, the front end leaves them to it
qc = fc.accepted("chain3")
twin = QuantumRegister(len(qc.qubits), qc.qregs[0].name)
ci = qc._data[0]
other = tuple(twin[qc.find_bit(q).index] for q in ci.qubits)
assert all(x == y and x is not y for x, y in zip(other, ci.qubits))
qc._data[0] = CircuitInstruction(ci.operation, other, ())
assert ing_mod._ingest_native.read_circuit(qc) is None
assert fc.declined_or_equal(qc) == "declined"

print("frontend strict worker ok")
