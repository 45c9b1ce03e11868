"""What scripts/ingest_native_asan (a host program built with -fsanitize=address,undefined, qcmrf_amd/csrc/ingest_native.cpp
compiled in; recipe in scripts/README.md) runs for the native back half of the front end: ``build_program`` on every accepted
circuit of tests/_frontend_cases.py for 1 / 2 / 4 / 8 shards and both layouts, held to ``planner.plan`` + ``program.encode``
on the way, and on the departures it must decline (arguments of the wrong type, shape, order or range), a few hundred
times each.  The built-in module stands in for qcmrf_amd._ingest_native.  No GPU."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
assert "_ingest_native" in sys.builtin_module_names, "run this with the program built from scripts/ingest_native_asan.cpp"
import _ingest_native
sys.modules["qcmrf_amd._ingest_native"] = _ingest_native

import numpy as np

from qcmrf_amd import frontend, program
from qcmrf_amd import ingest as ing_mod
from qcmrf_amd.backend import QsvBackend

import _frontend_cases as fc

assert ing_mod._ingest_native is _ingest_native and ing_mod.native_program_on()
native = _ingest_native.build_program
be = QsvBackend()


def arguments(qc, n_shards, layout):
    ing, opened, groups, shapes = frontend.front_half(qc, fc.dense_kmax_of(qc, n_shards))
    return [ing.num_qubits, opened, groups, [(k, m, np.multiply(m[..., 0], np.sqrt(2.0))) for k, _, m in shapes], n_shards, layout, 0.0]


n = 0
for name in sorted(fc.ACCEPTED):
    qc = fc.accepted(name)
    reps = 20 if qc.num_qubits > 20 else 100
    for n_shards in (1, 2, 4, 8):
        for layout in ("auto", "reference"):
            args = arguments(qc, n_shards, layout)
            fits = qc.num_qubits > n_shards.bit_length() - 1
            if fits:
                ing, ops = frontend.compile_blocks(qc, dense_kmax=fc.dense_kmax_of(qc, n_shards))
                pl = QsvBackend._plan(ing, ops, n_shards, dict(be.options, layout=layout))
                rec, data = program.encode(pl.ops)
                got = native(*args)
                assert bytes(got[1]) == rec.tobytes() and bytes(got[2]) == data.tobytes() and list(got[0]) == pl.layout
            for rep in range(reps):
                assert (native(*args) is not None) == fits
                n += 1

qc = fc.accepted("chain9")
good = arguments(qc, 1, "auto")
k, m, c0 = good[3][0]
declined = 0
for at, values in ((0, (0, 17, 65, -1, 18.0, None)), (1, (list(good[1]), good[1] + (99,), good[1] + (-1,), None)),
                   (2, ([], tuple(good[2]), good[2] + [None], good[2] + [good[2][0][:5]], good[2] + [(99,) + good[2][0][1:]])),
                   (3, ([], None, [(k, m)], [(k + 1, m, c0)], [(k, m[:-1], c0)], [(k, m, c0[:-1])], [(k, m.astype(np.complex64), c0)],
                        [(k, np.asfortranarray(m), c0)], [(k, np.concatenate([m, m])[::2], c0)], [(k, m.tolist(), c0)], [(k, m, None)],
                        [(k, m, c0), (k, m, c0)])),
                   (4, (0, 3, -2, 2.0, 1 << 18, 1 << 70)), (5, ("Auto", b"auto", None)), (6, (0.3, 0, None))):
    for value in values:
        args = list(good)
        args[at] = value
        for rep in range(300):
            assert native(*args) is None
            declined += 1
for junk in ((), (None,), tuple(good[:6]), tuple(good) + (None,)):
    for rep in range(300):
        assert native(*junk) is None
        declined += 1
for groups in ([None], [()], [(0, None, None, None, None, None)], [(0, [0, 1], None, None, None, None)]):
    for shapes in ([], good[3]):
        for rep in range(300):
            assert native(good[0], good[1], groups, shapes, 1, "auto", 0.0) is None
            declined += 1
assert native(*good) is not None
print("back half sanitizer run ok: %d programs built, %d calls declined" % (n, declined))
