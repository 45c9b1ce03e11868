"""What scripts/ingest_native_asan (a host program built with -fsanitize=address,undefined, qcmrf_amd/csrc/ingest_native.cpp
compiled in; recipe in scripts/README.md) runs for the native front end: ``read_circuit`` and ``frontend.compile_blocks`` on the
accepted circuits and on every departure from the grammar of tests/_frontend_cases.py, a few hundred times each.  The
built-in module stands in for qcmrf_amd._ingest_native.  No GPU."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
assert "_ingest_native" in sys.builtin_module_names, "run this with the program built from scripts/ingest_native_asan.cpp"
import _ingest_native
sys.modules["qcmrf_amd._ingest_native"] = _ingest_native

from qcmrf_amd import frontend
from qcmrf_amd import ingest as ing_mod

import _frontend_cases as fc

assert ing_mod._ingest_native is _ingest_native and ing_mod.native_frontend_on()

n = 0
for name in sorted(fc.ACCEPTED):
    qc = fc.accepted(name)
    fc.assert_accepted_and_equal(qc)
    for rep in range(20 if qc.num_qubits > 20 else 300):
        assert _ingest_native.read_circuit(qc) is not None
        n += 1
for spoil in fc.SPOILS:
    qc = fc.spoiled(spoil)
    how = fc.declined_or_equal(qc)
    for rep in range(300):
        assert (frontend.compile_blocks(qc) is None) == (how != "equal")
        n += 1
qc = fc.accepted("chain3")
qc.data = [(ci.operation, list(ci.qubits), list(ci.clbits)) for ci in qc.data]
for junk in (None, 3, "x", object(), [], {}, qc):
    for rep in range(300):
        assert _ingest_native.read_circuit(junk) is None
        n += 1
print("front end sanitizer run ok: %d circuit reads" % n)
