"""Writes the recorded references of the slow MEASURE cases (tests/_measure_cases.py, RECORDED) into
tests/golden/measure_refs/: ``exact_measure_sample`` of each case, with the digest of its inputs.

    python tests/golden/make_measure_refs.py [case name ...]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

import _measure_cases as mc          # noqa: E402


def main(names):
    os.makedirs(os.path.join(HERE, "measure_refs"), exist_ok=True)
    for name in names or sorted(mc.RECORDED):
        c = mc.case(name)
        words, alt_words, ambiguous, undetermined = mc.reference_of(c)
        np.savez_compressed(mc.recorded_path(name), words=words, alt_words=alt_words, ambiguous=ambiguous,
                            undetermined=undetermined, digest=np.array(mc.digest(c)), floats=mc.floats(c))
        print("%s: %d shots, %d ambiguous, %d undetermined" % (name, words.size, int(ambiguous.sum()), int(undetermined.sum())))


if __name__ == "__main__":
    main(sys.argv[1:])
