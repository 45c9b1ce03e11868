"""TEST INFRASTRUCTURE: one circuit ingested with the native block reader on and off, compared field by field
(tests/test_ingest_native.py, tests/_ingest_native_worker.py, tests/test_gpu_ingest_native.py)."""
import numpy as np

from qcmrf_amd import ingest as ing_mod
from qcmrf_amd.ingest import ingest

_OP_FIELDS = ("kind", "target", "ctrls", "vals", "qubits", "angle", "mask", "label", "cls", "a", "b", "new_pass")
_OP_ARRAYS = ("_mat", "_table", "mats")


def _same_array(x, y, what):
    if x is None or y is None:
        assert x is None and y is None, what
        return
    x, y = np.asarray(x), np.asarray(y)
    assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), what       # bit for bit


def assert_same(a, b):
    """two ``Ingested`` agree: op kinds, qubits and tables bit for bit, and everything the run reads besides"""
    assert (a.num_qubits, a.num_clbits) == (b.num_qubits, b.num_clbits)
    assert a.measure == b.measure and list(a.measure) == list(b.measure)
    assert a.global_phase == b.global_phase
    assert a.n_source_ops == b.n_source_ops
    assert a.creg_sizes == b.creg_sizes
    assert a.readout == b.readout and (a.n_pauli, a.n_kraus) == (b.n_pauli, b.n_kraus)
    assert (a.flat is None) == (b.flat is None)
    assert len(a.ops) == len(b.ops), (len(a.ops), len(b.ops))
    for k, (x, y) in enumerate(zip(a.ops, b.ops)):
        for f in _OP_FIELDS:
            assert getattr(x, f) == getattr(y, f), (k, f, getattr(x, f), getattr(y, f))
        for f in _OP_ARRAYS:
            _same_array(getattr(x, f), getattr(y, f), (k, f))


def both(circuit, **kw):
    """(Ingested with the native reader on, with it off); the switch is left as it was found"""
    was = ing_mod.use_native(True)
    try:
        a = ingest(circuit, peephole=True, **kw)
        ing_mod.use_native(False)
        b = ingest(circuit, peephole=True, **kw)
    finally:
        ing_mod.use_native(was)
    assert b.ingest_path == "python"
    return a, b


def both_raise(circuit, exc):
    """the text of the ``exc`` that ingest raises, the same with the native reader on and off"""
    texts = []
    was = ing_mod.use_native(True)
    try:
        for on in (True, False):
            ing_mod.use_native(on)
            try:
                ingest(circuit, peephole=True)
            except exc as e:
                texts.append(str(e))
            else:
                raise AssertionError("ingest (native=%s) did not raise %s" % (on, exc.__name__))
    finally:
        ing_mod.use_native(was)
    assert texts[0] == texts[1], texts
    return texts[0]


def blocks_of(circuit):
    """the definitions of the circuit's top-level composite instructions"""
    out = []
    for ci in circuit.data:
        op = ci.operation
        if op.name not in ing_mod._PRIMITIVES and op.name not in ("measure", "barrier"):
            d = getattr(op, "definition", None)
            if d is not None:
                out.append(d)
    return out


def assert_keys_equal(circuit, expect_native=True):
    """the native reader's (key, angles) against the Python reader's, definition by definition; returns how many blocks"""
    read = ing_mod._ingest_native.read_block
    n = 0
    for d in blocks_of(circuit):
        got, want = read(d), ing_mod._read_block(d)
        if not expect_native:
            assert got is None
            continue
        assert got is not None and want is not None
        key, lams = got
        assert type(key) is tuple and key == want[0] and hash(key) == hash(want[0])
        assert [type(x) for x in key] == [tuple] * 4
        assert all(type(x) is str for x in key[0]) and all(type(x) is int for x in key[1] + key[2])
        assert type(lams) is list and all(type(x) is float for x in lams)
        assert lams == [ing_mod._fparams(p)[0] for p in want[1]]
        n += 1
    return n
