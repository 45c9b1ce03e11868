"""What scripts/counts_native_asan (a host program built with -fsanitize=address,undefined, the counts formatter compiled in;
recipe in scripts/README.md) runs: the host cases of tests/test_counts_native.py -- every width, length, kind of words and
register list, the weighted merge, the off-path inputs, the fallbacks -- called as plain functions.  The built-in module
stands in for qcmrf_amd._counts_native.  No GPU."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
assert "_counts_native" in sys.builtin_module_names, "run this with the program built from scripts/counts_native_asan.cpp"
import _counts_native
sys.modules["qcmrf_amd._counts_native"] = _counts_native

from qcmrf_amd import backend as bk

assert bk._counts_native is _counts_native and bk.native_counts_available()

import test_counts_native as t

t.test_equals_python_dict()
t.test_top_bit_at_64_is_unsigned()
t.test_empty_and_num_clbits_zero()
for w in t.WIDTHS:
    t.test_weighted_equals_the_merge_it_replaces(w)
t.test_off_path_inputs_answer_none()
t.test_backend_falls_back_to_python()
t.test_switch()
t.test_a_wrong_formatter_fails_these_tests()
t.test_allocated_blocks_do_not_grow()
t.test_model_of_the_unshuffled_draw()
print("counts_native sanitizer run ok: %d cases x register lists, %d widths weighted" % (len(list(t.cases())), len(t.WIDTHS)))
