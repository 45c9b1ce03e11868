"""GPU box: what does ``run(..., noise_model=nm, accept=...)`` cost against running every attempt to its end and filtering on
the host?  (run from the root of the tree to measure)

    python scripts/time_noisy_accept.py [--case NAME] [--repeats 5] [--steps 5] [--attempts 20000]

Per case, in one process and alternately, ``--repeats`` windows of ``--steps`` steps each after two warm-up steps, each
window's mean, then the median and range over the windows:

  (a) plain + filter   ``run(shots=T)`` and the host filter on the fixed bits: what a tree without ``accept`` can do, with the
                       T it would have had to guess: T = the ``accept_attempts`` of (b)
  (b) accept           ``run(shots=S, accept=...)``; S is chosen so that T comes out near ``--attempts``: a probe of 4 accepted
                       shots gives the rate (under the thermal model the 10-variable chain accepts 1 attempt in 400, so S shots
                       are 400 S trajectories: 10 000 accepted shots would take minutes per step in (a))

A step ends in the counts on the host (synchronised).  Both legs do the same host compile per step; ``time_evolve`` -- the
metadata's time around the engine call, which ends in the copy of the words -- is reported beside the step time.  Also
reported: T, the share of attempts that an in-place measurement contradicts (abandoned in (b)), and the share of the records
of all T attempts that (b) skips, derived from the words of (a): a rejected attempt ends behind the first record, in program
order, that writes the final value of a fixed bit which contradicts.  1 - skipped share is what the time saved is to be
read against; it is a proxy: records differ in cost, and the final draw, which an abandoned attempt skips too, is no record
(the slot path, whose final draw is a pass of the whole workgroup over the state, can come out below it).

Cases: ``chain10`` the lowered 10-variable chain under thermal relaxation, depolarizing and readout errors, measurements in
place (12 live qubits, states in LDS); ``chain10-hbm`` the same with the states in device memory; ``cliques20`` 6 variables
on 20 pair cliques, constructed, 8 live qubits, where the model leaves about two attempts in a million accepted (the least
the case runs is 4 accepted shots, whatever ``--attempts`` says)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import _measure_cases as mc                            # noqa: E402  (the circuits and models of the tests)
from qcmrf_amd import QCMRF, _lib                      # noqa: E402
from qcmrf_amd.backend import QsvBackend               # noqa: E402


def chain10():
    fixed = QCMRF(mc.chain(10), mc.chain_theta(10), with_measurements=True).post_selection()
    return mc.chain_circuit(10), mc.lowered_model(), fixed


def cliques20():
    qc = mc.many_cliques()
    return qc, mc.constructed_model(), qc.post_selection()


CASES = {"chain10": (chain10, "lds"), "chain10-hbm": (chain10, "hbm"), "cliques20": (cliques20, "lds")}


def report(name, ms):
    print("  %-28s median %9.3f ms  range %9.3f .. %9.3f  windows %s"
          % (name, statistics.median(ms), min(ms), max(ms), " ".join("%.3f" % v for v in ms)), flush=True)
    return statistics.median(ms)


def skipped_share(rec, words, fixed):
    """(share of attempts abandoned, share of all records skipped) from the plain run's words"""
    at = {}                                            # fixed bit -> index of the last MEASURE record that writes it
    for k, r in enumerate(rec):
        if int(r["kind"]) == _lib.OP_MEASURE and int(r["vals"][0]) in fixed:
            at[int(r["vals"][0])] = k
    end = np.full(words.size, len(rec), dtype=np.int64)        # the record behind which the attempt ends
    for c, k in sorted(at.items(), key=lambda kv: -kv[1]):
        bad = ((words >> np.uint64(c)) & np.uint64(1)) != np.uint64(fixed[c])
        end[bad] = k + 1
    return float((end < len(rec)).mean()), float((len(rec) - end).sum() / (len(rec) * words.size))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default=None, choices=sorted(CASES))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--attempts", type=int, default=20000, help="attempts per step, about (the accepted shots follow from the rate)")
    args = ap.parse_args()
    for name in [args.case] if args.case else sorted(CASES):
        make, state = CASES[name]
        qc, nm, fixed = make()
        be = QsvBackend()
        opts = dict(seed_simulator=11, noise_model=nm, noisy_measure="in_place", noisy_state=state)
        probe = be.run(qc, shots=4, accept=fixed, accept_max_attempts=1 << 24, **opts).result().metadata()
        shots = max(4, int(round(args.attempts * 4 / probe["accept_attempts"])))
        opts["accept_max_attempts"] = 1 << 26              # (the plain leg does not look at it)
        first = be.run(qc, shots=shots, accept=fixed, **opts).result()
        m = first.metadata()
        T = m["accept_attempts"]
        prepared = QsvBackend._prepare_noisy(qc, nm, state, "in_place")
        rec, data, meas, readout = prepared[1], prepared[2], prepared[4], prepared[5]
        print("# %s: %d live qubits (%d in the circuit), %s, %d records of which %d MEASURE, %d shots accepted in T = %d attempts "
              "(estimate %.4g)" % (name, m["n_qubits"], m["n_circuit_qubits"], m["noisy_state"], len(rec), m["n_measure_ops"], shots, T,
                                   m["accept_probability"]), flush=True)
        with _lib.Engine(m["n_qubits"]) as eng:
            sample = eng.noisy_sample_hbm if state == "hbm" else eng.noisy_sample
            words = sample(rec, data, T, 11, meas, readout if prepared[0].readout else None)
        abandoned, skipped = skipped_share(rec, words, fixed)
        ok = np.ones(words.size, dtype=bool)
        for c, v in fixed.items():
            ok &= ((words >> np.uint64(c)) & np.uint64(1)) == np.uint64(v)
        assert int(ok.sum()) == shots and ok[-1], "the plain run of T shots does not hold exactly the accepted shots"

        def plain():
            res = be.run(qc, shots=T, **opts).result()
            counts = {k: v for k, v in res.get_counts().items() if all(k.replace(" ", "")[::-1][c] == str(v2) for c, v2 in fixed.items())}
            return counts, res.metadata()["time_evolve"] * 1e3

        def accept():
            res = be.run(qc, shots=shots, accept=fixed, **opts).result()
            return res.get_counts(), res.metadata()["time_evolve"] * 1e3

        assert plain()[0] == accept()[0] == first.get_counts(), "accept and the filtered plain run differ"
        legs = {"(a) plain + filter": plain, "(b) accept": accept}
        step_ms = {k: [] for k in legs}
        evolve_ms = {k: [] for k in legs}
        for leg in legs.values():
            leg()                                          # second warm-up step of each (the first was the comparison above)
        for _ in range(args.repeats):
            for k, leg in legs.items():                    # alternately: (a) window, (b) window, (a) window, ...
                ev = []
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    ev.append(leg()[1])
                step_ms[k].append((time.perf_counter() - t0) / args.steps * 1e3)
                evolve_ms[k].append(statistics.mean(ev))
        res = {}
        for k in legs:
            report(k + " step", step_ms[k])
            res[k] = report(k + " time_evolve", evolve_ms[k])
        a, b = res["(a) plain + filter"], res["(b) accept"]
        print("  attempts abandoned %.4f  records skipped %.4f  time_evolve (b) / (a) = %.3f  (bound from the records: %.3f)"
              % (abandoned, skipped, b / a, 1.0 - skipped), flush=True)
        be.close()


if __name__ == "__main__":
    main()
