"""CPU: the numpy restatement of the factored tile sums (_factored_sum_model.model_factored_sums) against math.fsum of
|amp|^2 of the amplitudes numpy forms, within _tile_sum_model.bound, on every program tests/test_gpu_factored_sums.py
runs; and every program has the |D| and the factor split it is built to have.  So the bound is known to hold for the
new order alone (its derivation is in _factored_sum_model)."""
import numpy as np
import pytest

import _factored_sum_model as fm
import _tile_sum_model as tm


@pytest.mark.parametrize("name", sorted(fm.CASES))
def test_model_within_the_bound(name):
    c = fm.CASES[name]
    tables = fm.tables_for(c["factors"], c["seed"], c["overrides"])
    amp, initval = fm.numpy_state(c["w"], c["zero"], c["factors"], tables)
    regs, _, block = tm.geometry(c["w"], c["r"], c["bit0"])
    want = tm.exact_tile_sums(amp, block)
    rel = tm.bound(len(c["factors"]), len(regs))
    for group in (-1, 0, 4):
        got = fm.model_factored_sums(c["w"], c["r"], c["bit0"], group, c["zero"], initval, c["factors"], tables)
        err = np.abs(got - want)
        assert (err <= rel * want).all(), (group, float((err / np.where(want > 0, want, 1)).max()) / rel)
        assert (got[want == 0.0] == 0.0).all()


@pytest.mark.parametrize("name", sorted(k for k, c in fm.CASES.items() if c["claim"]))
def test_claimed_split(name):
    c = fm.CASES[name]
    inner, uniform, d = fm.split(c["w"], c["r"], c["bit0"], c["zero"], c["factors"])
    assert (len(d), len(inner), len(uniform)) == c["claim"]
    assert len(inner) + len(uniform) == len(c["factors"])


def test_every_program_but_one_runs_factored():
    for name, c in fm.CASES.items():
        got = fm.info(c["w"], c["r"], c["bit0"], c["zero"], c["factors"], 1)
        assert got["factored"] == (name != "d4_no_uniform") and (got["uniform"] > 0) == (name != "d4_no_uniform"), (name, got)
    h = fm.CASES["hundred"]
    uniform = fm.split(16, 4, -1, h["zero"], h["factors"])[1]
    assert len(h["factors"]) == 100 and min(uniform) < 64 <= max(uniform)


def test_d_is_not_contiguous_at_18_and_20_qubits():
    for name, nblock in (("w18", 6), ("w20", 8)):
        c = fm.CASES[name]
        _, _, block = tm.geometry(c["w"], c["r"], c["bit0"])
        _, uniform, d = fm.split(c["w"], c["r"], c["bit0"], c["zero"], c["factors"])
        assert len(block) == nblock and [block.index(q) for q in d] == [0, 2, 5]
        assert max(len(c["factors"][k]) for k in uniform) == nblock


def test_zero_entries_make_zero_tiles():
    for name in ("zero_uniform_entry", "zero_inner_entry"):
        c = fm.CASES[name]
        tables = fm.tables_for(c["factors"], c["seed"], c["overrides"])
        amp, initval = fm.numpy_state(c["w"], c["zero"], c["factors"], tables)
        got = fm.model_factored_sums(c["w"], c["r"], c["bit0"], -1, c["zero"], initval, c["factors"], tables)
        assert ((got == 0.0).sum() > 0) == (name == "zero_uniform_entry")


def test_group_bits_stay_inside_d():
    for name, c in fm.CASES.items():
        _, _, d = fm.split(c["w"], c["r"], c["bit0"], c["zero"], c["factors"])
        for want in (-1, 0, 1, 2, 3, 4):
            g = fm.inner_group_bits(c["w"], c["r"], c["bit0"], c["zero"], c["factors"], want)
            assert set(g) <= set(d) and len(g) == min(3 if want < 0 else want, len(d), 4)
