"""Dynamic record streams on the MI355X: ``QSV_OP_IF`` and ``QSV_OP_RESET`` (include/qsv.h) through ``qsv_noisy_sample``,
``_hbm`` and ``_accept``.

The kernels that know the two kinds are held to the older ones word for word on static streams (engine option
``noisy_dynamic_kernels``), and to the Philox-exact reference of the contract (_dynamic_reference.py) word by word on streams
with the two kinds, at one width per kernel shape.  Comparisons with the reference go through ``check_kraus_words``:
undetermined plus ambiguous shots at most max(2, shots // 1000) per case (test_dynamic_reference.py asserts on the host that
every case stays within that cap on its own)."""
import numpy as np
import pytest

import _dynamic_cases as dc
import _kraus2_cases as k2c
from _dynamic_reference import check_kraus_words, dynamic_distribution, exact_dynamic_sample
from qcmrf_amd import _lib, get_backend, ir, program
from qcmrf_amd.backend import QsvBackend, _counts_of
from qcmrf_amd.noise import NoiseModel

pytestmark = pytest.mark.gpu


def sample(eng, c, hbm=False, shots=None):
    fn = eng.noisy_sample_hbm if hbm else eng.noisy_sample
    return fn(c["rec"], c["data"], c["shots"] if shots is None else shots, c["seed"], c["meas"], c["readout"])


# ---- 1. forced equality: the new kernels against the old ones on everything the old ones do -----------------------------------

def static_case(W):
    """a seeded random program of every unitary kind, PAULI, KRAUS and KRAUS2 records, with MEASURE records spliced in"""
    ops = k2c.random_ops(W, 8100 + W, 16 if W < 14 else 8)
    rng = np.random.RandomState(8200 + W)
    head = next(i for i, o in enumerate(ops) if o.kind != "init") + 1
    for q, c, release in ((0, 3, 0), (W // 2, 4, 1), (W - 1, 3, 0), (0, 5, 1)):
        ops.insert(int(rng.randint(head, len(ops) + 1)), dc.measure(q, c, release))
    rec, data = program.encode(ops)
    assert {_lib.OP_PAULI, _lib.OP_KRAUS, _lib.OP_KRAUS2, _lib.OP_MEASURE, _lib.OP_1Q, _lib.OP_MCX, _lib.OP_DIAG, _lib.OP_MCPHASE} <= set(rec["kind"].tolist())
    readout = np.zeros((6, 2))
    readout[:3] = [[0.03, 0.05], [0.0, 0.2], [0.1, 0.0]]
    return dict(W=W, rec=rec, data=data, shots=dc.SHOTS, seed=8300 + W, meas=[0, W // 2, W - 1, -1, -1, -1], readout=readout)


@pytest.mark.parametrize("W,hbm", [(3, False), (8, False), (11, False), (11, True), (14, True)])
def test_static_streams_run_the_same_words_through_the_dynamic_kernels(W, hbm):
    c = static_case(W)
    shots = c["shots"] if W < 14 else 512
    runs = []
    with _lib.Engine(W) as eng:
        for forced in (0, 1):
            eng.set_option("noisy_dynamic_kernels", forced)
            words = sample(eng, c, hbm, shots)
            kept, index, attempts = eng.noisy_sample_accept(c["rec"], c["data"], shots // 4, c["seed"], c["meas"], c["readout"], 1 << 3, 0,
                                                            hbm=hbm, max_attempts=shots)
            runs.append((words, kept, index, attempts))
        eng.set_option("noisy_dynamic_kernels", 0)
    (w0, k0, i0, a0), (w1, k1, i1, a1) = runs
    assert np.array_equal(w0, w1), "%d of %d words differ" % ((w0 != w1).sum(), w0.size)
    assert len(k0) > 0 and a0 == a1 and np.array_equal(k0, k1) and np.array_equal(i0, i1)
    assert len(set(w0.tolist())) > 4


# ---- 2. the two kinds, word by word against the exact reference ------------------------------------------------------------

@pytest.mark.parametrize("W,hbm", dc.SHAPES, ids=["W=%d %s" % (w, "slots" if h else "lds") for w, h in dc.SHAPES])
@pytest.mark.parametrize("name", sorted(dc.STREAMS))
def test_dynamic_stream_every_word(name, W, hbm):
    c = dc.stream_case(name, W)
    kinds = set(c["rec"]["kind"].tolist())
    assert kinds & {_lib.OP_IF, _lib.OP_RESET}
    with _lib.Engine(W) as eng:
        got = sample(eng, c, hbm)
    check_kraus_words(got, *dc.reference(name, W), family="dynamic", label="%s W=%d%s" % (name, W, " hbm" if hbm else ""))
    assert len(set(got.tolist())) > 1


# ---- 3. accept on a dynamic stream whose last writer of the fixed bit stands inside a span -------------------------------------

@pytest.mark.parametrize("W,hbm", dc.SHAPES, ids=["W=%d %s" % (w, "slots" if h else "lds") for w, h in dc.SHAPES])
@pytest.mark.parametrize("value", [0, 1])
def test_accept_with_the_decisive_record_inside_a_span(W, hbm, value):
    rec, data = program.encode(dc.accept_stream(W), n_meas=6)
    at = np.flatnonzero(rec["kind"] == _lib.OP_IF)[0]
    writers = [i for i in np.flatnonzero(rec["kind"] == _lib.OP_MEASURE) if int(rec["vals"][i, 0]) == 3]
    assert at < writers[-1] <= at + int(rec["n"][at]) and writers[0] < at         # the last writer of bit 3 is guarded
    meas, seed, shots = [0, W // 2, W - 1, -1, -1, -1], 6100 + W, 1000
    with _lib.Engine(W) as eng:
        kept, index, attempts = eng.noisy_sample_accept(rec, data, shots, seed, meas, None, 1 << 3, value << 3, hbm=hbm, max_attempts=dc.SHOTS)
        plain = (eng.noisy_sample_hbm if hbm else eng.noisy_sample)(rec, data, attempts, seed, meas, None)
    keep = np.flatnonzero(((plain >> np.uint64(3)) & np.uint64(1)) == np.uint64(value))
    assert 0 < len(kept) <= shots and attempts <= dc.SHOTS
    assert np.array_equal(index, keep[:len(kept)].astype(np.uint64)) and np.array_equal(kept, plain[keep][:len(kept)])
    ref = exact_dynamic_sample(rec, data, W, attempts, seed, meas, None)
    check_kraus_words(plain, *ref, family="dynamic accept", label="W=%d%s fixed to %d" % (W, " hbm" if hbm else "", value))


# ---- 4. end to end ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("state", ["lds", "hbm"])
@pytest.mark.parametrize("name", sorted(dc.CIRCUITS))
def test_run_dynamic_every_word(name, state):
    qc, nm, shots, seed = dc.CIRCUITS[name](), dc.readout_model(), dc.SHOTS, 4242
    backend = get_backend()
    res = backend.run(qc, shots=shots, seed_simulator=seed, noise_model=nm, dynamic=True, noisy_state=state).result()
    meta = res.metadata()
    ing, rec, data, clist, meas, readout, _, st, (mode, width, n_measure) = QsvBackend._prepare_noisy_dynamic(qc, nm, state)
    assert meta["dynamic"] is True and meta["noisy_state"] == state == st and meta["noisy_measure"] == mode == "in_place"
    assert meta["n_if_ops"] == int((rec["kind"] == _lib.OP_IF).sum()) and meta["n_reset_ops"] == int((rec["kind"] == _lib.OP_RESET).sum())
    assert meta["n_if_ops"] + meta["n_reset_ops"] > 0 or name == "active reset"
    with _lib.Engine(width) as eng:
        words = (eng.noisy_sample_hbm if state == "hbm" else eng.noisy_sample)(rec, data, shots, seed, meas, readout if ing.readout else None)
    assert _counts_of(words, None, ing.num_clbits, ing.creg_sizes)[0] == res.get_counts()
    ref = exact_dynamic_sample(rec, data, width, shots, seed, meas, readout if ing.readout else None)
    check_kraus_words(words, *ref, family="dynamic host path", label="%s %s" % (name, state))
    backend.close()


def test_run_dynamic_accept_is_the_filtered_run():
    qc, nm = dc.active_reset(), dc.readout_model()
    backend = get_backend()
    plain = backend.run(qc, shots=2000, seed_simulator=11, noise_model=nm, dynamic=True).result()
    kept = backend.run(qc, shots=200, seed_simulator=11, noise_model=nm, dynamic=True, accept={1: 0}).result()
    assert kept.metadata()["dynamic"] is True and 200 <= kept.metadata()["accept_attempts"] <= 2000
    assert all(k[0] == "0" for k in kept.get_counts()) and sum(kept.get_counts().values()) == 200
    assert set(kept.get_counts()) <= set(plain.get_counts())
    backend.close()


def test_density_matrix_runs_resets_exactly():
    qc, nm = dc.reset_only_circuit(), dc.readout_model()
    backend = get_backend()
    res = backend.run(qc, shots=1000, seed_simulator=5, noise_model=nm, dynamic=True, method="density_matrix").result()
    assert res.metadata()["dynamic"] is True and res.metadata()["n_reset_ops"] >= 1 and res.metadata()["method"] == "density_matrix"
    ing, rec, data, clist, meas, readout, _, st, (mode, width, n_measure) = QsvBackend._prepare_noisy_dynamic(qc, nm, "lds")
    want = dynamic_distribution(rec, data, width, meas, readout if ing.readout else None)
    got = np.zeros(want.size)
    for k, p in res.get_probabilities().items():
        got[int(k.replace(" ", ""), 2)] = p
    print("density vs dynamic_distribution: max |dp| = %.3e" % np.abs(got - want).max())
    assert np.abs(got - want).max() < 1e-10 and abs(got.sum() - 1.0) < 1e-10
    assert sum(res.get_counts().values()) == 1000
    backend.close()


# ---- the refusals of the library: by message, before any launch ----------------------------------------------------------------

def raw(*rows):
    rec = np.zeros(len(rows), dtype=_lib.OP_DTYPE)
    for r, row in zip(rec, rows):
        for k, v in row.items():
            if k in ("qubits", "vals"):
                r[k][:len(v)] = v
            else:
                r[k] = v
    return rec


def IF(span, mask, value=0, negate=0):
    halves = np.array([value & 0xFFFFFFFF, value >> 32], dtype=np.uint32).view(np.int32)
    return dict(kind=_lib.OP_IF, n=span, mask=mask, vals=[int(halves[0]), int(halves[1])], target=negate)


X0 = dict(kind=_lib.OP_MCX, target=0, n=0)
RESET0 = dict(kind=_lib.OP_RESET, n=1, qubits=[0])


@pytest.mark.parametrize("rows,meas,match", [
    ([IF(0, 1, 1), X0], [0, -1], "op 0: QSV_OP_IF guards a span of 0"),
    ([IF(2, 1, 1), X0], [0, -1], "op 0: QSV_OP_IF guards 2 records, 1 follow"),
    ([IF(1, 0, 0), X0], [0, -1], "op 0: QSV_OP_IF compares no classical bit"),
    ([IF(1, 2, 3), X0], [0, -1], "op 0: QSV_OP_IF value 0x3 has bits outside its mask"),
    ([IF(1, 4, 4), X0], [0, -1], "op 0: QSV_OP_IF mask 0x4 reads a classical bit outside the 2 bits"),
    ([IF(1, 2, 2), X0], None, "op 0: QSV_OP_IF reads classical bits and needs meas_qubits"),
    ([IF(2, 2, 2), IF(1, 2, 2), X0], [0, -1], "op 1: QSV_OP_IF inside the span of the QSV_OP_IF record 0"),
    ([IF(1, 2, 2), dict(kind=_lib.OP_INIT_ZERO)], [0, -1], "op 1: an INIT record inside the span of the QSV_OP_IF record 0"),
    ([IF(1, 2, 2, 2), X0], [0, -1], "op 0: QSV_OP_IF negate flag 2"),
    ([dict(kind=_lib.OP_RESET, n=1, qubits=[3])], [0, -1], "QSV_OP_RESET"),
], ids=["span 0", "span past the end", "mask 0", "value outside mask", "mask past n_meas", "no map", "if in span", "init in span",
        "negate", "reset qubit"])
def test_library_refuses_by_message(rows, meas, match):
    with _lib.Engine(3) as eng:
        for fn in (eng.noisy_sample, eng.noisy_sample_hbm):
            with pytest.raises(ValueError, match=match):
                fn(raw(*rows), np.zeros(2), 16, 1, meas)
        with pytest.raises(ValueError, match=match):
            eng.noisy_sample_accept(raw(*rows), np.zeros(2), 16, 1, meas)


def test_other_entry_points_refuse_the_two_kinds():
    with _lib.Engine(4) as eng:
        for rows, match in (([IF(1, 2, 2), X0], "QSV_OP_IF"), ([RESET0], "QSV_OP_RESET")):
            with pytest.raises(ValueError, match=match + ".*not in qsv_exec"):
                eng.exec(raw(*rows), np.zeros(2))
            for fn in (eng.density_exec, eng.density_exec_accept):
                with pytest.raises(RuntimeError, match=match):
                    fn(raw(*rows), np.zeros(2))
