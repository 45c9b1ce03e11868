"""Cases, reference and stand-in engine of the tests of ``qsv_noisy_sample_accept`` (test infrastructure): noisy shots kept
only when fixed bits of their word read given values.

The reference is the rule of include/qsv.h applied to ``exact_measure_sample``: attempt t is shot t; it is accepted iff
(word & fix_mask) == fix_val; the call returns the first ``shots`` accepted attempts.  ``PLANS`` names every seeded case the
GPU tests run; test_accept_host.py asserts for each that the flagged shots (ambiguous or undetermined) of its window stay
within the project's cap and that none lies among the attempts the call examines, so that ``attempts`` can be asserted."""
from __future__ import annotations

import functools

import numpy as np

import _kraus_cases as kc
import _measure_cases as mc
import _noise_exact_cases as nc
from _measure_reference import MeasureNumpyEngine, exact_measure_sample
from qcmrf_amd import _lib, ir, program


def mask_of(fixed):
    """{bit: 0 | 1} -> (fix_mask, fix_val)"""
    fm = fv = 0
    for c, v in fixed.items():
        fm |= 1 << c
        fv |= int(v) << c
    return fm, fv


def accepts(words, fixed):
    fm, fv = mask_of(fixed)
    return (np.asarray(words, dtype=np.uint64) & np.uint64(fm)) == np.uint64(fv)


# ---- record-level cases ---------------------------------------------------------------------------------------------------
# The MEASURE records of a ``_measure_cases`` program write the bits of CLBITS = (0, 31, 32, 63), each of them twice (the last
# write decides); its register reads the bits 1, 2, 5, 30, 33, 40, 62 in the final draw.

@functools.lru_cache(maxsize=None)
def slot_case(W, shots, n_random):
    """``_measure_cases.random_case`` at a width it has no table entry for (the slot path's 12 and 15)"""
    rng = np.random.RandomState(7000 + W)
    base = nc.random_ops(W, 7100 + W, n_random=n_random, init="uniform" if W % 2 else None)
    for q in mc.slots(W)[:2]:
        base.insert(int(rng.randint(W + 1, len(base) + 1)), kc.kraus_op(q, kc.isometry_kraus(rng, 1 + q % 4)))
    rec, data = program.encode(mc.with_measures(base, W, rng))
    meas, ro = mc.register(W, rng)
    return dict(W=W, rec=rec, data=data, shots=shots, seed=7700 + W, meas=meas, readout=ro)


@functools.lru_cache(maxsize=None)
def case_and_reference(name):
    """(case, (words, alt_words, ambiguous, undetermined)) over the case's window, first_shot = 0; computed once, shared"""
    if name.startswith("slot W="):
        W = int(name.split("=")[1])
        c = slot_case(W, *{12: (400, 6), 15: (96, 4)}[W])
        ref = mc.reference_of(c)
        for a in ref:
            a.setflags(write=False)
        return c, ref
    return mc.case(name), mc.reference(name)


# name -> (path, [fixed bits, ...]): the widths at which the kernel forms change (LDS: fewer amplitudes than lanes, the last
# width with one pair per lane, eight pairs per lane, the last one-wave width, workgroups, the LDS limit; slot path 4, 12, 15)
PLANS = {
    "lds W=3": ("lds", [{63: 1}, {0: 0, 31: 1}]),
    "lds W=7": ("lds", [{0: 1}, {31: 0, 32: 0, 63: 0}]),
    "lds W=8": ("lds", [{63: 0}, {32: 1, 5: 0}]),
    "lds W=10": ("lds", [{32: 1, 63: 0}, {0: 0}]),
    "lds W=11": ("lds", [{31: 1}, {0: 0, 32: 1, 62: 0}]),
    "lds W=13": ("lds", [{32: 0}, {31: 1, 63: 1}]),
    "grids": ("hbm", [{63: 0}, {0: 1, 31: 1, 63: 1}]),                       # W = 4
    "slot W=12": ("hbm", [{32: 1}, {0: 0, 32: 0}]),
    "slot W=15": ("hbm", [{63: 0}, {63: 1, 2: 0}]),
}


def plan(name, fixed):
    """what the reference says about ``accept`` of case ``name`` with the bits ``fixed``: the shots asked for (half of what
    its window accepts, so that the call ends inside the window), the accepted indices, the attempts examined, the flagged
    shots among them and in the whole window"""
    c, (words, alt, amb, undet) = case_and_reference(name)
    ok = accepts(words, fixed)
    flagged = amb | undet
    shots = max(1, int(ok.sum()) // 2)
    index = np.flatnonzero(ok)[:shots]
    attempts = int(index[-1]) + 1 if index.size == shots else words.size
    return dict(case=c, shots=shots, index=index, words=words[index], attempts=attempts, accepted=ok, flagged=flagged,
                flagged_examined=int(flagged[:attempts].sum()), ref=(words, alt, amb, undet))


def check_accept(got, p, label):
    """(words, indices, attempts) of a call against ``plan``: per attempt index over the examined window every determined
    shot is accepted iff the reference accepts it, with the reference's word; ``attempts`` equal where no examined shot
    is flagged"""
    words, index, attempts = got
    ref_words, alt, amb, undet = p["ref"]
    assert len(words) == len(index) == p["shots"], "%s: %d of %d shots accepted" % (label, len(words), p["shots"])
    assert (np.diff(index.astype(np.int64)) > 0).all(), "%s: indices not ascending" % label
    assert attempts == int(index[-1]) + 1, "%s: attempts %d, last accepted index %d" % (label, attempts, int(index[-1]))
    assert attempts <= ref_words.size, "%s: %d attempts leave the window of %d" % (label, attempts, ref_words.size)
    taken = np.zeros(ref_words.size, dtype=bool)
    taken[index.astype(np.int64)] = True
    sure = ~p["flagged"]
    sure[attempts:] = False
    wrong = np.flatnonzero(sure & (taken != p["accepted"]))
    assert wrong.size == 0, "%s: attempt %d is %s, the reference says otherwise (word %#x)" % (
        label, wrong[0], "accepted" if taken[wrong[0]] else "rejected", int(ref_words[wrong[0]]))
    at = index.astype(np.int64)
    bad = np.flatnonzero(sure[at] & (words != ref_words[at]))
    assert bad.size == 0, "%s: attempt %d accepted with word %#x, reference %#x" % (
        label, at[bad[0]], int(words[bad[0]]), int(ref_words[at[bad[0]]]))
    unsure = np.flatnonzero(~sure[at])                               # a flagged shot that was accepted: one of its two words
    for j in unsure:
        if not undet[at[j]]:
            assert words[j] in (ref_words[at[j]], alt[at[j]]), "%s: ambiguous attempt %d" % (label, at[j])
    print("ACCEPT case=%s shots=%d attempts=%d (reference %d) flagged among them=%d" % (label, p["shots"], attempts, p["attempts"],
                                                                                      p["flagged_examined"]))
    if p["flagged_examined"] == 0:
        assert attempts == p["attempts"], "%s: %d attempts, the reference examines %d" % (label, attempts, p["attempts"])
        assert np.array_equal(index.astype(np.int64), p["index"]) and np.array_equal(words, p["words"]), label


# ---- forced outcomes: deterministic, no reference -------------------------------------------------------------------------

def forced_accept_programs(W):
    """(label, (rec, data), meas, readout, fixed, all accepted?) on the last qubit of a W-qubit state: outcomes that are
    certain, so a call accepts every attempt or none"""
    s, none = W - 1, [-1] * 64
    x, m = ir.op_x(s), mc.measure_op
    for release in (1, 0):
        tag = "release" if release else "no release"
        yield "X, measure, fixed to 0, " + tag, program.encode([x, m(s, 63, release, (0.0, 0.0))]), none, None, {63: 0}, False
        yield "X, measure, fixed to 1, " + tag, program.encode([x, m(s, 63, release, (0.0, 0.0))]), none, None, {63: 1}, True
        # acceptance is on the bit that was read: the qubit is 1, the readout surely flips it
        yield "X, measure read as 0, fixed to 0, " + tag, program.encode([x, m(s, 63, release, (0.0, 1.0))]), none, None, {63: 0}, True
        yield "X, measure read as 0, fixed to 1, " + tag, program.encode([x, m(s, 63, release, (0.0, 1.0))]), none, None, {63: 1}, False
    # a bit written twice: only its last write may end a shot
    twice = [x, m(s, 63, 1, (0.0, 0.0)), m(s, 63, 0, (0.0, 0.0))]                  # 1, then 0 over it
    yield "1 then 0, fixed to 0", program.encode(twice), none, None, {63: 0}, True
    yield "1 then 0, fixed to 1", program.encode(twice), none, None, {63: 1}, False
    twice = [m(s, 63, 0, (0.0, 0.0)), x, m(s, 63, 1, (0.0, 0.0))]                  # 0, then 1 over it
    yield "0 then 1, fixed to 0", program.encode(twice), none, None, {63: 0}, False
    yield "0 then 1, fixed to 1", program.encode(twice), none, None, {63: 1}, True
    # a fixed bit that the final draw writes: nothing to abandon, the filter alone
    final = list(none)
    final[7] = s
    yield "X, final draw, fixed to 0", program.encode([x]), final, None, {7: 0}, False
    yield "X, final draw, fixed to 1", program.encode([x]), final, None, {7: 1}, True
    ro = np.zeros((64, 2))
    ro[7] = (0.0, 1.0)
    yield "X, final draw read as 0, fixed to 0", program.encode([x]), final, ro, {7: 0}, True
    # both: the record agrees, the final draw decides
    both = [x, m(s, 63, 0, (0.0, 0.0))]
    yield "record agrees, final draw contradicts", program.encode(both), final, None, {63: 1, 7: 0}, False
    yield "record agrees, final draw agrees", program.encode(both), final, None, {63: 1, 7: 1}, True


# ---- the exact stand-in engine --------------------------------------------------------------------------------------------

class AcceptExactEngine(MeasureNumpyEngine):
    """MeasureNumpyEngine whose noisy entry points are the Philox-exact reference (``exact_measure_sample``), shot by shot,
    and which implements ``noisy_sample_accept`` from it by the rule of include/qsv.h, in rounds"""

    rounds = []                    # the attempts of every launch-like round, for the tests of ``round``

    def _sample(self, limit, ops, data, shots, seed, meas_qubits, readout, first_shot=0):
        if self.n_qubits > limit:
            raise ValueError("noisy shots: at most %d qubits" % limit)
        if not shots:
            return np.zeros(0, dtype=np.uint64)
        return exact_measure_sample(ops, data, self.n_qubits, shots, seed, meas_qubits, readout, first_shot=first_shot)[0]

    def noisy_sample_accept(self, ops, data, shots, seed, meas_qubits=None, readout=None, fix_mask=0, fix_val=0, first_shot=0,
                            max_attempts=None, round=0, hbm=False):
        shots = int(shots)
        if max_attempts is None:
            max_attempts = max(2 ** 20, 1000 * shots)
        if shots and not max_attempts:
            raise ValueError("qsv: max_attempts = 0")
        limit = _lib.NOISY_HBM_MAX_QUBITS if hbm else _lib.NOISY_MAX_QUBITS
        ahead = np.zeros(0, dtype=np.uint64)     # the reference walks the program per call: attempts are computed 256 at a time
        words, index, examined = [], [], 0       # and handed out round by round
        while len(words) < shots and examined < max_attempts:
            n = min(int(round) or max(shots, 64), max_attempts - examined)
            AcceptExactEngine.rounds.append(n)
            while ahead.size < n:
                more = self._sample(limit, ops, data, max(256, n - ahead.size), seed, meas_qubits, readout, first_shot + examined + ahead.size)
                ahead = np.concatenate([ahead, more])
            w, ahead = ahead[:n], ahead[n:]
            hit = np.flatnonzero((w & np.uint64(fix_mask)) == np.uint64(fix_val))[:shots - len(words)]
            words += w[hit].tolist()
            index += (hit + first_shot + examined).tolist()
            examined += int(hit[-1]) + 1 if len(words) == shots else n
        return np.array(words, dtype=np.uint64), np.array(index, dtype=np.uint64), examined
