"""What scripts/ingest_native_asan (a host program built with -fsanitize=address,undefined, the block reader compiled in;
recipe in scripts/README.md) runs: the reader on the circuits of tests/test_ingest_native.py, fast path and fallbacks,
a few hundred times each.  The built-in module stands in for qcmrf_amd._ingest_native.  No GPU."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
assert "_ingest_native" in sys.builtin_module_names, "run this with the program built from scripts/ingest_native_asan.cpp"
import _ingest_native
sys.modules["qcmrf_amd._ingest_native"] = _ingest_native

from qcmrf_amd import QCMRF, workloads
from qcmrf_amd import ingest as ing_mod
from qcmrf_amd.ingest import ingest

assert ing_mod._ingest_native is _ingest_native and ing_mod.native_available()


def theta(c):
    return workloads.theta_halfnorm(workloads.dimension(c))


def blocks(qc):
    return [ci.operation.definition for ci in qc.data if ci.operation.name.startswith("cU_C")]


def tuples(qc):
    d = blocks(qc)[0]
    d.data = [(ci.operation, list(ci.qubits), list(ci.clbits)) for ci in d.data]


def bad_param(qc):
    blocks(qc)[0].data[1].operation.params = [object()]


def no_condition(qc):
    for d in blocks(qc):
        for ci in d.data:
            del ci.operation.condition


def raising(qc):
    class Raises:
        name = "and"
        condition = None
        params = ()

        @property
        def definition(self):
            raise RuntimeError("no definition today")
    d = blocks(qc)[0]
    d.data[0] = type(d.data[0])(Raises(), d.data[0].qubits, ())


n = 0
for cliques in ([[0, 1]], [[0, 1, 2]], workloads.chain(4), workloads.baseline_config(4)[1]):
    for spoil in (None, tuples, bad_param, no_condition, raising):
        qc = QCMRF(cliques, theta(cliques))
        if spoil is not None:
            spoil(qc)
        for rep in range(300 if len(cliques) < 5 else 20):
            for d in blocks(qc):
                got = _ingest_native.read_block(d)
                if got is not None:
                    assert got[0] == ing_mod._read_block(d)[0]
                n += 1
            try:
                ingest(qc, peephole=True)
            except (ValueError, RuntimeError):
                assert spoil in (bad_param, raising)
for junk in (None, 3, "x", object(), [], {}):
    assert _ingest_native.read_block(junk) is None
print("ingest_native sanitizer run ok: %d block reads" % n)
