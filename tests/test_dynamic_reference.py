"""The references of the dynamic-circuit tests against closed forms, against each other, and against deliberately wrong
versions of themselves (no GPU): what test_gpu_noisy_dynamic.py leans on."""
import numpy as np
import pytest

import _dynamic_cases as dc
import _kraus2_cases as k2c
from _dynamic_reference import MUTATIONS, dynamic_distribution, exact_dynamic_sample, within_cap
from qcmrf_amd import ir, mrf, program
from qcmrf_amd.backend import QsvBackend
from qcmrf_amd.noise import NoiseModel

H = ir.FIXED_1Q["h"]


def dist_of(ops, W, meas, readout=None):
    rec, data = program.encode(ops, n_meas=len(meas))
    return dynamic_distribution(rec, data, W, meas, readout)


@pytest.mark.parametrize("f0,f1", [(0.0, 0.0), (0.11, 0.23), (0.5, 0.02), (1.0, 0.3)])
def test_active_reset_leaves_one_with_half_the_flip_sum(f0, f1):
    ops = [ir.op_u(0, H), dc.measure(0, 0, flips=(f0, f1)), dc.guard(1, 1, 1), ir.op_x(0)]
    d = dist_of(ops, 1, [-1, 0])
    assert abs(d[2] + d[3] - 0.5 * (f0 + f1)) < 1e-12 and abs(d.sum() - 1.0) < 1e-12
    # the recorded first bit reads 1 in half of the shots whatever the flips are symmetric or not: (1 - f1 + f0) / 2
    assert abs(d[1] + d[3] - 0.5 * (1.0 - f1 + f0)) < 1e-12


def test_reset_after_h_gives_zero():
    d = dist_of([ir.op_u(0, H), dc.reset(0)], 1, [0])
    assert np.abs(d - [1.0, 0.0]).max() < 1e-12
    # and it keeps the other qubit's marginal when the two were entangled
    d = dist_of([dc.ry(0, 1.2), dc.cx(0, 1), dc.reset(0)], 2, [0, 1])
    assert np.abs(d - [np.cos(0.6) ** 2, 0.0, np.sin(0.6) ** 2, 0.0]).max() < 1e-12


def test_gate_on_a_bit_never_written_does_not_run():
    d = dist_of([dc.guard(1, 1 << 1, 1 << 1), ir.op_x(0)], 1, [0, -1])
    assert np.abs(d - [1.0, 0.0, 0.0, 0.0]).max() < 1e-12
    d = dist_of([dc.guard(1, 1 << 1, 1 << 1, 1), ir.op_x(0)], 1, [0, -1])        # negated: it runs
    assert np.abs(d - [0.0, 1.0, 0.0, 0.0]).max() < 1e-12


def test_shared_ancilla_circuit_gives_the_distribution_of_the_original():
    qc, src = dc.shared_ancilla_qcmrf()
    ing, rec, data, clist, meas, readout, _, state, (mode, width, n_measure) = QsvBackend._prepare_noisy_dynamic(qc, NoiseModel(), "lds")
    assert width == src.num_vertices + 2 and mode == "in_place" and ing.n_reset == len(dc.CHAIN3) - 1    # the last reset is dropped
    d = dynamic_distribution(rec, data, width, meas, None)
    want = k2c.exact_distribution(src, None)
    assert np.abs(d - want).max() < 1e-12
    n = src.num_vertices
    p, _ = mrf.gibbs_pmf(dc.CHAIN3, dc.CHAIN3_THETA)
    ok = d[:1 << n]
    assert np.abs(ok / ok.sum() - p).max() < 1e-12
    assert abs(ok.sum() - mrf.success_probability(dc.CHAIN3, dc.CHAIN3_THETA)) < 1e-12


def small_streams():
    """streams of at most 16 recorded words"""
    yield "active reset", [ir.op_u(0, H), dc.measure(0, 0), dc.guard(1, 1, 1), ir.op_x(0)], 1, [-1, 0], np.array([[0.0, 0.0], [0.05, 0.1]])
    yield ("reset in a span", [dc.ry(0, 1.1), dc.cx(0, 1), dc.measure(0, 2), dc.guard(2, 1 << 2, 1 << 2), dc.pauli(1, 0.3, 0.1, 0.1),
                               dc.reset(0), dc.ry(0, 0.4)], 2, [0, 1, -1], None)
    yield ("every kind", [dc.ry(0, 0.9), dc.ry(1, 1.3), dc.measure(0, 2), dc.guard(4, 1 << 2, 0), dc.pauli(1, 0.2, 0.1, 0.1), dc.damping(1, 0.4),
                          dc.damping2(0, 1, 0.5), dc.measure(1, 3), dc.pauli(0, 0.3, 0.1, 0.2), dc.reset(1), dc.ry(1, 0.5)], 2, [0, 1, -1, -1], None)


@pytest.mark.parametrize("name,ops,W,meas,readout", list(small_streams()), ids=[s[0] for s in small_streams()])
def test_sampler_follows_the_distribution(name, ops, W, meas, readout):
    S = 65536
    rec, data = program.encode(ops, n_meas=len(meas))
    p = dynamic_distribution(rec, data, W, meas, readout)
    assert abs(p.sum() - 1.0) < 1e-12 and p.size <= 16
    words, _, _, _ = exact_dynamic_sample(rec, data, W, S, 20261020, meas, readout)
    count = np.bincount(words.astype(np.int64), minlength=p.size)
    assert count.size == p.size, "a word outside the distribution's support"
    bound = 5.0 * np.sqrt(S * p * (1.0 - p)) + 1.0
    print(name, np.c_[count, S * p, bound])
    assert (np.abs(count - S * p) <= bound).all()


@pytest.mark.parametrize("W", sorted({w for w, _ in dc.SHAPES}))
def test_every_case_stays_within_the_ambiguity_cap(W):
    for name in dc.STREAMS:
        _, _, amb, undet = dc.reference(name, W)
        n, cap = within_cap(amb, undet)
        print(name, W, n, cap)
        assert cap == 4 and n <= cap, "%s at W = %d: %d undetermined or ambiguous shots (cap %d): change its angles" % (name, W, n, cap)


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_every_mutation_is_seen_by_some_case(mutation):
    seen = []
    for name in dc.STREAMS:
        ref = dc.reference(name, 3)
        bad = dc.reference_of(dc.stream_case(name, 3), _mutate=mutation)
        sure = ~(ref[2] | ref[3] | bad[2] | bad[3])
        if (ref[0][sure] != bad[0][sure]).any():
            seen.append(name)
    print(mutation, seen)
    assert seen, "no case of the suite tells %r from the contract" % mutation
