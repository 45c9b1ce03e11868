"""Drop-in for the simulator call of the reference:

    simulator = Aer.get_backend('qasm_simulator')          /root/reference/run_experiment.py:54
    result    = simulator.run(T, shots=SHOTS).result()     /root/reference/run_experiment.py:56
    counts    = result.get_counts()                        /root/reference/run_experiment.py:57

``run`` accepts one circuit or a list, nested (un-transpiled ``QCMRF`` objects) or lowered to
``{cx,id,rz,sx,x}``; counts come back as plain ``{bitstring: int}`` dicts (classical bit W-1
leftmost), a list of them when more than one circuit ran -- ``json.dumps``-able as
run_experiment.py:59-61 requires.

Execution = ingest -> exact fusion passes -> layout/shard plan -> ONE ``qsv_exec`` call into
libqsv.so (hand-written HIP, gfx950) -> probability pass + sampling on the device.  There is no
host-side simulation path: without the library or a GPU, ``run`` raises.
"""
from __future__ import annotations

import time

import numpy as np

from . import _lib, frontend, ingest as _ingest, noise as _noise, passes, planner, program
from .comm import SingleProcess

_METHODS = ("statevector", "trajectory", "density_matrix")
_WALKS = ("depth", "levels")
_NOISY_STATES = ("lds", "hbm", "auto")
_NOISY_MEASURES = ("deferred", "in_place", "auto")
_DENSITY_MEASURES = ("deferred", "in_place", "auto")
DENSITY_MAX_CLBITS = 20       # method="density_matrix" returns 2^k probabilities over the k written classical bits

_NAMES = ("qasm_simulator", "aer_simulator", "aer_simulator_statevector", "statevector_simulator",
          "qsv_simulator")


class Result:
    def __init__(self, experiments, backend_name):
        self._exps = experiments
        self.backend_name = backend_name
        self.success = True
        self.time_taken = sum(e["metadata"]["time_taken"] for e in experiments)

    @property
    def results(self):
        return self._exps

    def get_counts(self, experiment=None):
        if experiment is None:
            cs = [dict(e["counts"]) for e in self._exps]
            return cs[0] if len(cs) == 1 else cs
        if isinstance(experiment, int):
            return dict(self._exps[experiment]["counts"])
        for e in self._exps:
            if e["name"] == getattr(experiment, "name", experiment):
                return dict(e["counts"])
        raise KeyError("no experiment %r" % (experiment,))

    def get_probabilities(self, experiment=None):
        """exact distribution over the written classical bits, ``{bitstring: p}`` with the keys of ``get_counts`` and the
        entries with p > 0 only (``method="density_matrix"`` runs; a list when more than one circuit ran)"""
        def one(e):
            if "probabilities" not in e:
                raise ValueError("experiment %r holds no exact distribution: run it with method='density_matrix'" % (e["name"],))
            return dict(e["probabilities"])
        if experiment is None:
            ps = [one(e) for e in self._exps]
            return ps[0] if len(ps) == 1 else ps
        if isinstance(experiment, int):
            return one(self._exps[experiment])
        for e in self._exps:
            if e["name"] == getattr(experiment, "name", experiment):
                return one(e)
        raise KeyError("no experiment %r" % (experiment,))

    def metadata(self, i=0):
        return self._exps[i]["metadata"]

    def to_dict(self):
        return {"backend_name": self.backend_name, "success": True,
                "results": [{"name": e["name"], "shots": e["shots"], "counts": e["counts"],
                             "metadata": e["metadata"]} for e in self._exps]}


class Job:
    def __init__(self, result):
        self._result = result

    def result(self):
        return self._result

    def status(self):
        return "DONE"


def _format_keys(values, counts, num_clbits, creg_sizes):
    """integer outcomes (bit c = classical bit c) -> Qiskit count keys, vectorised:
    one (keys x width) matrix of '0'/'1' bytes, decoded once and sliced"""
    w = max(num_clbits, 1)
    wide = getattr(values, "dtype", None) == object  # registers past 64 bits: Python ints (trajectory mode)
    if not wide:
        values = np.ascontiguousarray(values, dtype=np.uint64)
    if wide:
        keys = [format(int(v), "0%db" % w) for v in values]
    elif w <= 64:
        # big-endian bytes -> bits -> UCS4 code points '0'/'1', VIEWED as fixed-width strings: no
        # per-key conversion at all (an S -> U astype costs more than everything else here together)
        bits = np.unpackbits(values.astype(">u8").view(np.uint8).reshape(-1, 8), axis=1)[:, 64 - w:]
        code = np.empty(bits.shape, dtype=np.uint32)
        np.add(bits, 48, out=code, casting="unsafe")
        keys = code.view("<U%d" % w).ravel().tolist()
    else:
        shifts = np.arange(w - 1, -1, -1, dtype=np.uint64)
        chars = (((values[:, None] >> np.minimum(shifts, np.uint64(63))) & np.uint64(1)) * (shifts < 64) + np.uint64(48)).astype(np.uint8)
        text = chars.tobytes().decode("ascii")
        keys = [text[i * w:(i + 1) * w] for i in range(len(values))]
    if creg_sizes and len(creg_sizes) > 1:           # one group per register, last register first
        cuts, hi = [], num_clbits
        for _, size in reversed(creg_sizes):
            cuts.append((num_clbits - hi, num_clbits - hi + size))
            hi -= size
        keys = [" ".join(k[a:b] for a, b in cuts) for k in keys]
    return dict(zip(keys, counts.tolist()))


try:
    from . import _counts_native          # built by qcmrf_amd.build next to libqsv.so; absent where Python's headers are missing
except Exception:                         # not built, or does not load here: counts are sorted and formatted in Python (same dict)
    _counts_native = None
_native_counts = _counts_native.counts_dict if _counts_native is not None else None


def native_counts_available():
    """the native counts formatter was built and loads"""
    return _counts_native is not None


def use_native_counts(on=True):
    """force the switch: sampled words become the count dict in the native formatter (``on``; RuntimeError where it is not
    available) or through ``np.unique`` and ``_format_keys``.  Returns the previous setting.  The default is on wherever
    the module imports.  Either way the dict is the same, insertion order included."""
    global _native_counts
    was = _native_counts is not None
    if on and _counts_native is None:
        raise RuntimeError("qcmrf_amd._counts_native is not built or does not import (python -m qcmrf_amd.build)")
    _native_counts = _counts_native.counts_dict if on else None
    return was


def _counts_path_default():
    """metadata ``counts_path`` of a run that had no words to count: what the switch says"""
    return "native" if _native_counts is not None else "python"


def _counts_of(words, weights, num_clbits, creg_sizes):
    """(the count dict of ``words``, the path that built it): keys in ascending order of the words, a word's count the
    number of times it occurs, or the sum of its ``weights`` (int64, one per word) where those are given.  The native
    formatter where it is on and takes the input (it answers None and decides nothing otherwise), else ``_format_keys``."""
    if _native_counts is not None:
        got = _native_counts(words, weights, num_clbits, creg_sizes)
        if got is not None:
            return got, "native"
    if weights is None:
        uv, uc = np.unique(words, return_counts=True)
    else:
        # the same word can come from several parts
        uv, inv = np.unique(words, return_inverse=True)
        uc = np.bincount(inv, weights=weights, minlength=uv.size).astype(np.int64) if uv.size != words.size else weights[np.argsort(words, kind="stable")]
    return _format_keys(uv, uc, num_clbits, creg_sizes), "python"


class QsvBackend:
    """MI355X statevector backend.  Options (constructor or per ``run`` call):

    fusion      0 gate by gate | 1 + init/diagonal fusion | 2 + multiplexer fusion |
                3 + dense <=5-qubit windows with structure recovery (default)
    fold_fresh  (fusion 3) gates whose target nothing has touched yet become factors of the
                initial product state, written in the same pass as the state itself (default on)
    layout      'auto' (exchange-free where possible) | 'reference' (qubit q on index bit q)
    devices     HIP device id per shard owned by this process (repeat an id for virtual shards)
    method      'statevector' (default: all measurements deferred, one evolution, W qubits) |
                'trajectory' (mid-circuit measurements taken when they occur, measured qubits
                released: n+2 live qubits for a QCMRF circuit, see qcmrf_amd.trajectory; classical registers of any
                width) |
                'density_matrix' (the circuit under ``noise_model``, or ideal, evolved exactly as rho -> sum K rho K^dg in a
                vector of 2W qubits: ``Result.get_probabilities()`` is the exact distribution over the written classical
                bits, the counts are drawn from it; W <= 17, one process, <= 20 written classical bits)
    trajectory_walk   (method 'trajectory') 'depth' (default: one engine per branch of the outcome tree, depth first) |
                'levels' (the live branches of a level are the slots of one wider state: one program launch, one
                ``qsv_branch_mass`` and one vectorised binomial draw per batch, one ``qsv_branch_split`` per run of children).
                The two walks draw in different orders: for one seed their counts agree statistically, not shot by shot
    trajectory_slots  (walk 'levels') branches of a batch at most, a power of two; None (default): 2^30 bytes worth, halved
                while segments + 2 engines of that size exceed 80 % of the free device memory; counts are a function of
                (circuit, shots, seed, fusion, resolved slots); a value that cannot fit is a MemoryError
    trajectory_trace  (walk 'levels', per run call) a list that receives one record per measuring batch: (level, register bits,
                shots, mass on 0, mass on 1, shots on 1), each per slot -- for tests that replay the draws
    comm        process group for one-process-per-GPU launches (qcmrf_amd.comm)
    gather_counts  'root' (default: rank 0 returns the merged counts, the other ranks an empty dict) | 'all'
    spmd_ingest    (multi-rank) each rank reads 1/N of the circuit's composite blocks, one all-gather completes the program
                   (default off: in the only rehearsal available -- ranks sharing one GPU -- the extra collective cost more
                   than the reading it saved)
    device      HIP device of this rank when ``comm`` is given
    noise_model a ``qcmrf_amd.noise.NoiseModel`` (Pauli and one-qubit Kraus gate errors, readout errors): every shot is its own trajectory
                on the device (``qsv_noisy_sample``), W <= 13 qubits and <= 64 classical bits; None or an empty model
                runs the ideal path
    noisy_state where a noisy shot keeps its state: 'lds' (default: on-chip memory, W <= 13) | 'hbm' (a slot of device
                memory per resident shot, ``qsv_noisy_sample_hbm``, W <= 24; the same draws and words) | 'auto' ('lds' up to
                13 qubits, 'hbm' above); resolved on the live width when the measurements are taken in place
    noisy_measure  when a noisy shot measures: 'deferred' (default: every measurement at the end, one qubit per clique ancilla,
                W = n + m + 1 for a QCMRF circuit) | 'in_place' (a mid-circuit measurement is taken when it occurs, as one
                QSV_OP_MEASURE record, and its qubit recycled: n + 2 live qubits for any number of cliques; the trailing
                measurements stay one joint final draw; same limits: <= 64 classical bits; reset, gates after a measure and
                classical conditions need ``dynamic``) | 'auto' (in place iff that makes the state narrower).  A shot's Pauli,
                Kraus and readout draws are the same in both; 'density_matrix' has ``density_measure`` instead
    density_measure  (method 'density_matrix' only) when rho is measured: 'deferred' (default: every measurement at the end,
                W = n + m + 1 for a QCMRF circuit, W <= 17 and <= 20 written classical bits) | 'in_place' (a mid-circuit
                measurement whose bit ``accept`` fixes is applied where it occurs, as the one linear map "read the accepted
                value, hand the qubit back in |0>" (``qsv_density_exec_accept``), and its qubit recycled: n + 2 live qubits for
                any number of cliques; the limits hold for the live width and for the bits of the trailing measurements,
                which stay the final read-out of the diagonal; every mid-circuit bit must be fixed by ``accept`` and written
                once, otherwise a ValueError names the bit) | 'auto' (in place iff that is possible and makes rho narrower).
                ``accept_probability`` and ``get_probabilities()`` mean what they mean deferred; metadata gains
                ``density_measure`` (resolved), ``n_qubits`` (live), ``n_circuit_qubits`` and ``n_measure_ops``
    accept      (noisy runs and method 'density_matrix') ``{classical bit: 0 | 1}``, or a list with one dict per circuit
                (``QCMRF.post_selection()`` is a valid value): only shots whose bits read these values are kept, and ``shots`` is
                the number of KEPT shots.  A noisy run takes attempts 0, 1, 2, ... -- attempt t is shot t of the same run without
                ``accept`` -- and keeps the first ``shots`` that match (``qsv_noisy_sample_accept``); an attempt is abandoned on
                the device as soon as a measurement taken in place contradicts, so ``noisy_measure='auto'`` or 'in_place' is
                what saves work (deferred: every attempt runs to its end and is filtered).  Metadata: ``accept``,
                ``accept_attempts`` and ``accept_probability`` = (shots - 1) / (attempts - 1), the unbiased estimate of the
                success rate when sampling stops at the shots-th success (1 / attempts for one shot) -- functions of (circuit,
                model, seed, shots) alone.  'density_matrix': ``get_probabilities()`` is the exact distribution conditioned on
                the fixed bits (readout confusion included), ``accept_probability`` the exact mass of the condition, the counts
                ``numpy.random.default_rng(seed).multinomial(shots, p)``.  Not ``post_select``, which conditions the exact state
                vector of an ideal run and refuses noise; giving both is an error
    accept_max_attempts  attempts examined at most (default max(2^20, 1000 shots)); a RuntimeError names the rate seen if they
                run out
    accept_round  attempts per launch (default 0: chosen by the library); no result depends on it
    dynamic     False (default: every run as it is without the option) | True: a circuit that holds a ``reset``, a classically
                conditioned instruction (``c_if``, ``if_test`` / ``if_else`` with an optional else body; equality of a bit or a
                register with an integer) or a gate on a qubit measured earlier runs shot by shot on the device, under
                ``noise_model`` or under an empty model when none is given (``QSV_OP_IF``, ``QSV_OP_RESET``; the noise ops of a
                conditioned gate lie inside its guard, so its error occurs only when the gate does).  Measurements are taken in
                place (metadata ``noisy_measure`` 'in_place'), ``noisy_state`` resolves on the live width (13 on chip, 24 in
                slots), ``accept`` works as on any noisy run; metadata gains ``dynamic``, ``n_if_ops`` and ``n_reset_ops``.  A
                circuit without any of it runs as without the option.  method 'density_matrix' runs resets exactly (conditions
                and a measured qubit used again without a reset would need branching: ValueError).  Still refused, by a
                ValueError that says why: ``post_select``, method 'trajectory', ``comm`` of several ranks, more than one
                device, more than 64 classical bits, nested conditions, loops and ``switch``
    """

    def __init__(self, name="qasm_simulator", **options):
        self._name = name
        self.options = {"fusion": 3, "layout": "auto", "devices": (0,), "comm": None, "device": 0,
                        "profile": False, "engine_options": None, "method": "statevector", "fold_fresh": True,
                        "gather_counts": "root", "noise_model": None, "noisy_state": "lds", "noisy_measure": "deferred",
                        "trajectory_walk": None, "trajectory_slots": None, "trajectory_trace": None}
        self.options.update(options)
        self._engine = None
        self._engine_key = None
        self.last_engine = None
        self.last_plan = None
        self._last_comm = None
        self._engine_factory = None      # test hook only; the default and only shipped engine is libqsv

    def name(self):
        return self._name

    def set_options(self, **options):
        self.options.update(options)

    # ---- engine cache: re-use the device allocation across circuits of one width ---------
    def _get_engine(self, n_qubits, opts):
        comm = opts["comm"] or SingleProcess()
        if comm.world > 1:
            key = (n_qubits, "rank", comm.rank, comm.world, opts["device"])
        else:
            key = (n_qubits, tuple(opts["devices"]))
        if self._engine is not None and self._engine_key == key:
            return self._engine
        if self._engine is not None:
            self._engine.close()
            self._engine = None
        make = self._engine_factory or _lib.Engine
        if comm.world > 1:
            eng = make(n_qubits, devices=(opts["device"],), rank=comm.rank, world_size=comm.world)
            eng._comm_ready = False
        else:
            eng = make(n_qubits, devices=tuple(opts["devices"]))
            eng._comm_ready = True
        self._engine, self._engine_key = eng, key
        return eng

    def statevector(self):
        """amplitudes left by the last run, in LOGICAL qubit order (diagnostic; copies 2^W values
        to the host, so small circuits only).  Index bit q = logical qubit q."""
        eng, pl = self.last_engine, self.last_plan
        amp = eng.amplitudes()
        p = np.arange(amp.size, dtype=np.int64)
        l = np.zeros_like(p)
        for q, pos in enumerate(pl.layout):
            l |= ((p >> pos) & 1) << q
        out = np.empty_like(amp)
        out[l] = amp
        return out

    def expectation_diagonal(self, diag, qubits, fixed=None):
        """(sum |amp|^2 diag[j], sum |amp|^2) over the basis states in which every qubit of ``fixed``
        ({logical qubit: 0/1}) has the given value, on the state the LAST run left in HBM; ``diag`` is
        a real diagonal over the logical ``qubits`` (index bit b <-> qubits[b]).  The first divided by
        the second is the expectation in the post-selected state.  One read pass on the device
        (qsv_expect_diag); summed over the ranks of a multi-process run.  Replaces the opflow
        expectation of QCMRF.Hamiltonian() / sufficient_statistic() (QCMRF.py:159-193)."""
        eng, pl = self.last_engine, self.last_plan
        if eng is None or pl is None:
            raise RuntimeError("expectation_diagonal needs a state: run() a circuit on this backend first")
        phys = [pl.layout[q] for q in qubits]
        fm = fv = 0
        for q, v in (fixed or {}).items():
            fm |= 1 << pl.layout[q]
            fv |= int(bool(v)) << pl.layout[q]
        s0, s1 = eng.expect_diag(phys, np.ascontiguousarray(diag, dtype=np.float64), fm, fv)
        comm = self._last_comm
        if comm is not None and comm.world > 1:
            parts = comm.allgather((s0, s1))
            s0, s1 = sum(p[0] for p in parts), sum(p[1] for p in parts)
        return s0, s1

    def marginals(self, groups, fixed=None):
        """(list of arrays, mass) on the state the LAST run left: for every group of logical qubits the 2^k sums of
        |amp|^2 over the basis states in which every qubit of ``fixed`` ({logical qubit: 0/1}) has the given value and
        the group's qubits spell the bin (bin bit b <-> group[b]); ``mass`` is the sum over all those states.  Not
        normalised.  One pass over the matching amplitudes for all groups (qsv_marginals_cond); a deferred state whose
        fixed bits select tiles stays deferred.  One process only, as post_select; virtual shards are fine."""
        eng, pl = self.last_engine, self.last_plan
        if eng is None or pl is None:
            raise RuntimeError("marginals needs a state: run() a circuit on this backend first")
        comm = self._last_comm
        if comm is not None and comm.world > 1:
            raise ValueError("marginals runs in one process; this state is spread over %d ranks" % comm.world)
        phys = [[pl.layout[q] for q in g] for g in groups]
        fm = fv = 0
        for q, v in (fixed or {}).items():
            fm |= 1 << pl.layout[q]
            fv |= int(bool(v)) << pl.layout[q]
        return eng.marginals_cond(phys, fm, fv)

    def top_states(self, k, fixed=None):
        """(logical indices uint64, p) on the state the LAST run left: the k most probable basis states in which every
        qubit of ``fixed`` ({logical qubit: 0/1}) has the given value, by descending p = |amp|^2, equal p by ascending
        logical index; only states with p > 0.  Not normalised.  One pass over the matching amplitudes
        (qsv_top_cond), exact; a deferred state whose fixed bits select tiles stays deferred.  The engine selects in
        the PHYSICAL index order of the run's layout and the indices are un-permuted here: with states tied exactly at
        the k-th place, which of them are returned is decided by the physical order (the returned pairs are still
        sorted by (-p, logical index)); without such a tie the result does not depend on the layout.  One process only,
        as post_select; virtual shards are fine."""
        eng, pl = self.last_engine, self.last_plan
        if eng is None or pl is None:
            raise RuntimeError("top_states needs a state: run() a circuit on this backend first")
        comm = self._last_comm
        if comm is not None and comm.world > 1:
            raise ValueError("top_states runs in one process; this state is spread over %d ranks" % comm.world)
        fm = fv = 0
        for q, v in (fixed or {}).items():
            fm |= 1 << pl.layout[q]
            fv |= int(bool(v)) << pl.layout[q]
        phys, p = eng.top_cond(k, fm, fv)
        phys = np.asarray(phys, dtype=np.uint64)
        moved = [(q, b) for q, b in enumerate(pl.layout) if q != b]          # (most of a layout is the identity)
        logical = phys & np.uint64(sum(1 << b for q, b in enumerate(pl.layout) if q == b))
        for q, b in moved:
            logical |= ((phys >> np.uint64(b)) & np.uint64(1)) << np.uint64(q)
        order = np.lexsort((logical, -np.asarray(p, dtype=np.float64)))
        return logical[order], np.asarray(p, dtype=np.float64)[order]

    def marginals_rows(self, groups, fixed_rows):
        """(out (B, nbins), mass (B,)) on the state the LAST run left: ``marginals(groups, fixed_rows[r])`` for every row
        of ``fixed_rows`` (a sequence of {logical qubit: 0/1}) from ONE device pass -- one conditional query per data row
        of a model.  Row r of ``out`` holds the groups' bins one after the other and equals the single call's byte for
        byte (qsv_marginals_cond_rows); a deferred state stays deferred where the bits all rows fix alike select tiles.
        One process only, as ``marginals``; virtual shards are fine."""
        eng, pl = self.last_engine, self.last_plan
        if eng is None or pl is None:
            raise RuntimeError("marginals_rows needs a state: run() a circuit on this backend first")
        comm = self._last_comm
        if comm is not None and comm.world > 1:
            raise ValueError("marginals_rows runs in one process; this state is spread over %d ranks" % comm.world)
        phys = [[pl.layout[q] for q in g] for g in groups]
        bit = [1 << p for p in pl.layout]
        masks, vals = [], []
        for fixed in fixed_rows:
            fm = fv = 0
            for q, v in (fixed or {}).items():
                fm |= bit[q]
                if v:
                    fv |= bit[q]
            masks.append(fm)
            vals.append(fv)
        return eng.marginals_cond_rows(phys, masks, vals)

    def close(self):
        if self._engine is not None:
            self._engine.close()
            self._engine = None

    # ---- the call run_experiment.py:56 makes -------------------------------------------------
    def run(self, circuits, shots=1024, seed_simulator=None, **run_options):
        opts = dict(self.options)
        opts.update(run_options)
        single = not isinstance(circuits, (list, tuple))
        circs = [circuits] if single else list(circuits)
        if seed_simulator is None:
            seed_simulator = int(np.random.SeedSequence().entropy % (2 ** 63))
        exps = []
        method = opts.get("method", "statevector")
        if method not in _METHODS:
            raise ValueError("unknown method %r; this backend runs %s" % (method, ", ".join(_METHODS)))
        walk, tslots = opts.get("trajectory_walk"), opts.get("trajectory_slots")
        if walk is not None and walk not in _WALKS:
            raise ValueError("unknown trajectory_walk %r; the outcome tree is walked by %s" % (walk, " or ".join(map(repr, _WALKS))))
        ttrace = opts.get("trajectory_trace")
        if method != "trajectory" and (walk is not None or tslots is not None or ttrace is not None):
            raise ValueError("trajectory_walk, trajectory_slots and trajectory_trace belong to method='trajectory', not method=%r" % (method,))
        if ttrace is not None and walk != "levels":
            raise ValueError("trajectory_trace records the batches of the walk by 'levels'; the walk by 'depth' has none")
        if ttrace is not None and not isinstance(ttrace, list):
            raise TypeError("trajectory_trace must be a list, not %s" % type(ttrace).__name__)
        state = opts.get("noisy_state", "lds")
        if state not in _NOISY_STATES:
            raise ValueError("unknown noisy_state %r; a noisy shot keeps its state in %s" % (state, ", ".join(_NOISY_STATES)))
        nmeasure = opts.get("noisy_measure", "deferred")
        if nmeasure not in _NOISY_MEASURES:
            raise ValueError("unknown noisy_measure %r; a noisy shot takes its measurements %s" % (nmeasure, ", ".join(_NOISY_MEASURES)))
        dmeasure = opts.get("density_measure")
        if dmeasure is not None and dmeasure not in _DENSITY_MEASURES:
            raise ValueError("unknown density_measure %r; a density matrix takes its measurements %s" % (dmeasure, ", ".join(_DENSITY_MEASURES)))
        if dmeasure is not None and method != "density_matrix":
            raise ValueError("density_measure belongs to method='density_matrix', not method=%r (noisy shots have noisy_measure)" % (method,))
        if opts.get("dynamic"):
            feats = [_ingest.ingest(c, dynamic=True) for c in circs]
            if any(f.n_if or f.n_reset or f.n_reuse for f in feats):
                return Job(Result(self._run_dynamic(circs, feats, int(shots), int(seed_simulator), opts, run_options, method, state,
                                                    dmeasure), self._name))
        accept = self._accept_of(opts, len(circs), method)      # (first: it is the one that refuses the two together)
        post = self._post_select_of(opts, len(circs), method)
        if method == "density_matrix":
            if nmeasure == "in_place":
                raise ValueError("method='density_matrix' defers every measurement; noisy_measure='in_place' belongs to noisy shots")
            model = self._density_model_of(opts)
            from concurrent.futures import ThreadPoolExecutor
            with ThreadPoolExecutor(max_workers=1) as pool:     # host compile of circuit i+1 while the device evolves circuit i
                prepare = lambda i: self._prepare_density_measure(circs[i], model, dmeasure, accept and accept[i])     # noqa: E731
                nxt = pool.submit(prepare, 0)
                for i in range(len(circs)):
                    prepared, place = nxt.result()
                    if i + 1 < len(circs):
                        nxt = pool.submit(prepare, i + 1)
                    exps.append(self._run_density(circs[i], int(shots), int(seed_simulator) + i, opts, prepared,
                                                  accept=accept and accept[i], place=place))
            return Job(Result(exps, self._name))
        model = self._noise_of(opts)
        if model is not None:
            # host compile of circuit i+1 on a helper thread while the device runs the shots of circuit i
            from concurrent.futures import ThreadPoolExecutor
            with ThreadPoolExecutor(max_workers=1) as pool:
                nxt = pool.submit(self._prepare_noisy, circs[0], model, state, nmeasure)
                for i in range(len(circs)):
                    prepared = nxt.result()
                    if i + 1 < len(circs):
                        nxt = pool.submit(self._prepare_noisy, circs[i + 1], model, state, nmeasure)
                    exps.append(self._run_noisy(circs[i], int(shots), int(seed_simulator) + i, opts, prepared,
                                                accept=accept and accept[i]))
            return Job(Result(exps, self._name))
        if len(circs) > 1 and opts.get("method", "statevector") == "statevector":
            # a batch (run_experiment.py:52-56 hands over 70 circuits): compile circuit i+1 on a
            # helper thread while the device evolves and samples circuit i (ctypes releases the GIL
            # inside the blocking library calls)
            from concurrent.futures import ThreadPoolExecutor
            opts = dict(opts, _batch=True)          # (the helper thread must not talk on the process group's socket: no SPMD ingest here)
            with ThreadPoolExecutor(max_workers=1) as pool:
                nxt = pool.submit(self._prepare, circs[0], opts)
                for i in range(len(circs)):
                    prepared = nxt.result()
                    if i + 1 < len(circs):
                        nxt = pool.submit(self._prepare, circs[i + 1], opts)
                    exps.append(self._run_one(circs[i], int(shots), int(seed_simulator) + i, opts, prepared, post_select=post and post[i]))
        else:
            for i, c in enumerate(circs):
                exps.append(self._run_one(c, int(shots), int(seed_simulator) + i, opts, post_select=post and post[i]))
        return Job(Result(exps, self._name))

    def _post_select_of(self, opts, n_circuits, method):
        """the ``post_select`` option as one ``{classical bit: 0 | 1}`` per circuit, or None; refuses what the
        post-selected sampler does not cover"""
        post = opts.get("post_select")
        if post is None:
            return None
        if method != "statevector":
            raise ValueError("post_select belongs to method='statevector', not method=%r" % (method,))
        if self._noise_of(opts) is not None:
            raise ValueError("post_select takes no noise_model: the conditioned state of a noisy run is not a state vector")
        comm = opts["comm"] or SingleProcess()
        if comm.world > 1:
            raise ValueError("post_select takes one process (a process group of %d ranks was given; limit 1)" % comm.world)
        if isinstance(post, dict):
            post = [post] * n_circuits
        post = list(post)
        if len(post) != n_circuits or not all(isinstance(d, dict) for d in post):
            raise ValueError("post_select is one {classical bit: 0 | 1} dict, or a list of %d of them (one per circuit)" % n_circuits)
        return post

    def _accept_of(self, opts, n_circuits, method):
        """the ``accept`` option as one ``{classical bit: 0 | 1}`` per circuit, or None; refuses the runs that have no shots
        to reject"""
        accept = opts.get("accept")
        if accept is None:
            return None
        if opts.get("post_select") is not None:
            raise ValueError("accept and post_select were both given: post_select conditions the exact state vector of an ideal "
                             "run, accept keeps the shots of a noisy run whose bits match")
        if method == "trajectory":
            raise ValueError("accept belongs to noisy runs and method='density_matrix', not method='trajectory'")
        comm = opts["comm"] or SingleProcess()
        if comm.world > 1:
            raise ValueError("accept takes one process (a process group of %d ranks was given; limit 1)" % comm.world)
        if method == "statevector" and self._noise_of(opts) is None:
            raise ValueError("accept keeps the shots of a noisy run whose bits match; an ideal state-vector run has an exact "
                             "conditioned state: use post_select")
        if isinstance(accept, dict):
            accept = [accept] * n_circuits
        accept = list(accept)
        if len(accept) != n_circuits or not all(isinstance(d, dict) for d in accept):
            raise ValueError("accept is one {classical bit: 0 | 1} dict, or a list of %d of them (one per circuit)" % n_circuits)
        return accept

    @staticmethod
    def _accept_mask(accept, ing):
        """(fix_mask, fix_val) over the classical bits (bit c of a recorded word is classical bit c)"""
        fm = fv = 0
        for c, v in accept.items():
            if c not in ing.measure:
                raise ValueError("accept names classical bit %r, which no measurement writes" % (c,))
            if v not in (0, 1):
                raise ValueError("accept fixes classical bit %r to %r; a bit reads 0 or 1" % (c, v))
            fm |= 1 << int(c)
            fv |= int(v) << int(c)
        return fm, fv

    @staticmethod
    def _post_select_mask(post, ing, pl):
        """(fix_mask, fix_val) over the physical index bits: classical bit -> the qubit measured into it -> its position"""
        fixed = {}
        for c, v in post.items():
            if c not in ing.measure:
                raise ValueError("post_select names classical bit %r, which no measurement writes" % (c,))
            if v not in (0, 1):
                raise ValueError("post_select fixes classical bit %r to %r; a bit reads 0 or 1" % (c, v))
            q = ing.measure[c]
            if fixed.setdefault(q, int(v)) != int(v):
                raise ValueError("post_select fixes qubit %d (classical bit %r) to both 0 and 1" % (q, c))
        fm = fv = 0
        for q, v in fixed.items():
            fm |= 1 << pl.layout[q]
            fv |= v << pl.layout[q]
        return fm, fv

    @staticmethod
    def _noise_of(opts):
        """the noise model a run has to honour, or None (no model, or one without any error: the ideal path)"""
        model = opts.get("noise_model")
        if model is None:
            return None
        if not isinstance(model, _noise.NoiseModel):
            raise TypeError("noise_model must be a qcmrf_amd.noise.NoiseModel, not %s" % type(model).__name__)
        if model.is_ideal():
            return None
        if opts.get("method", "statevector") == "trajectory":
            raise ValueError("method='trajectory' cannot be combined with a noise model (noisy runs are per-shot trajectories "
                             "of at most %d qubits already)" % _lib.NOISY_MAX_QUBITS)
        comm = opts["comm"] or SingleProcess()
        if comm.world > 1:
            raise ValueError("noisy runs take one process (a process group of %d ranks was given; limit 1)" % comm.world)
        return model

    @staticmethod
    def _resolve_noisy_state(state, width, what):
        """the run option noisy_state resolved ('lds' or 'hbm') for a per-shot state of ``width`` qubits"""
        if state == "auto":
            state = "lds" if width <= _lib.NOISY_MAX_QUBITS else "hbm"
        if state == "lds" and width > _lib.NOISY_MAX_QUBITS:
            raise ValueError("noisy runs keep one state per shot in on-chip memory: at most %d qubits, the circuit has %d%s "
                             "(noisy_state='hbm' or 'auto' keeps it in device memory: at most %d qubits)"
                             % (_lib.NOISY_MAX_QUBITS, width, what, _lib.NOISY_HBM_MAX_QUBITS))
        if state == "hbm" and width > _lib.NOISY_HBM_MAX_QUBITS:
            raise ValueError("noisy runs with noisy_state='hbm' keep one state per shot in device memory: at most %d qubits, "
                             "the circuit has %d%s" % (_lib.NOISY_HBM_MAX_QUBITS, width, what))
        return state

    @staticmethod
    def _prepare_noisy(circuit, model, state="lds", measure="deferred"):
        """host half of a noisy run: ingest with the model's Pauli and Kraus ops (identity layout) + encode; ``state`` and
        ``measure`` are the run options noisy_state and noisy_measure, returned resolved ('lds' or 'hbm'; 'deferred' or
        'in_place')"""
        t0 = time.perf_counter()
        if measure != "deferred":
            prepared = QsvBackend._prepare_noisy_in_place(circuit, model, state, measure == "auto", t0)
            if prepared is not None:
                return prepared
        ing = _ingest.ingest(circuit, noise=model)
        state = QsvBackend._resolve_noisy_state(state, ing.num_qubits, "")
        if ing.num_clbits > 64:
            raise ValueError("noisy runs record at most 64 classical bits, the circuit has %d" % ing.num_clbits)
        rec, data = program.encode(ing.ops)
        clist = sorted(ing.measure)
        meas = [-1] * (clist[-1] + 1) if clist else []
        readout = np.zeros((len(meas), 2))
        for c in clist:
            meas[c] = ing.measure[c]
            readout[c] = ing.readout.get(c, (0.0, 0.0))
        return ing, rec, data, clist, meas, readout, time.perf_counter() - t0, state, ("deferred", ing.num_qubits, 0)

    @staticmethod
    def _prepare_noisy_in_place(circuit, model, state, only_if_narrower, t0):
        """``_prepare_noisy`` with the mid-circuit measurements taken when they occur: the ops of the deferred ingest, Pauli
        and Kraus ops included, in their order and remapped to live slots (``trajectory.plan_slots``), every mid-circuit
        measure a "measure" op (one QSV_OP_MEASURE record, its flips those of the measured logical qubit), the trailing
        ones one joint final draw through ``meas`` (-1 for the bits written earlier).  None: ``only_if_narrower`` and the
        live width is the circuit's"""
        from . import ir, trajectory
        ing = _ingest.ingest(circuit, noise=model, keep_measures=True)
        if ing.num_clbits > 64:
            raise ValueError("noisy runs record at most 64 classical bits, the circuit has %d" % ing.num_clbits)
        staged, width, finals = trajectory.plan_slots(ing.ops)
        width = max(width, 1)
        if only_if_narrower and width >= ing.num_qubits:
            return None
        state = QsvBackend._resolve_noisy_state(state, width, " live at once with its measurements taken in place")
        early = {item[2] for item in staged if item[0] == "measure"}
        late = [(s, c) for s, c in finals if c in early]    # a bit written earlier and again at the end: a record as well, so
        finals = [(s, c) for s, c in finals if c not in early]   # that the last write wins
        ops, n_measure = [], 0
        for item in staged:
            if item[0] == "ops":
                ops += item[1]
            else:
                _, s, c, release, q = item
                ops.append(ir.Op("measure", target=s, mask=c, vals=(int(release),), table=model.readout_flips(q)))
                n_measure += 1
        for s, c in late:
            ops.append(ir.Op("measure", target=s, mask=c, vals=(0,), table=ing.readout.get(c)))
            n_measure += 1
        ing.ops = ops
        rec, data = program.encode(ops)
        clist = sorted(ing.measure)
        meas = [-1] * (clist[-1] + 1) if clist else []
        readout = np.zeros((len(meas), 2))
        for s, c in finals:
            meas[c] = s
            readout[c] = ing.readout.get(c, (0.0, 0.0))
        return ing, rec, data, clist, meas, readout, time.perf_counter() - t0, state, ("in_place", width, n_measure)

    def _run_noisy(self, circuit, shots, seed, opts, prepared, accept=None):
        """one qsv_noisy_sample (or qsv_noisy_sample_hbm) call: shots trajectories, sampled and read out on the device;
        ``accept``: one qsv_noisy_sample_accept call, shots accepted trajectories"""
        ing, rec, data, clist, meas, readout, t_compile, state, (nmeasure, width, n_measure) = prepared
        t1 = time.perf_counter()
        t0 = t1 - t_compile
        counts = {}
        counts_path = _counts_path_default()
        t2 = t1
        fix = None if accept is None else self._accept_mask(accept, ing)
        accept_meta = {} if fix is None else {"accept": dict(accept), "accept_attempts": 0, "accept_probability": None}
        if clist and shots > 0:
            eng = self._get_engine(width, dict(opts, comm=None, devices=tuple(opts["devices"])[:1]))
            self._apply_engine_options(eng, opts)
            if fix is not None:
                limit = opts.get("accept_max_attempts")
                limit = max(2 ** 20, 1000 * shots) if limit is None else int(limit)
                bits, _, attempts = eng.noisy_sample_accept(rec, data, shots, seed, meas, readout if ing.readout else None, fix[0], fix[1],
                                                            0, limit, int(opts.get("accept_round") or 0), state == "hbm")
                if len(bits) < shots:
                    raise RuntimeError("accept %r: %d attempts made, %d of %d shots accepted (rate seen %.3g); accept_max_attempts "
                                       "sets the limit" % (accept, attempts, len(bits), shots, len(bits) / max(attempts, 1)))
                accept_meta.update(accept_attempts=attempts,
                                   accept_probability=(shots - 1) / (attempts - 1) if shots > 1 else 1.0 / attempts)
            else:
                sample = eng.noisy_sample_hbm if state == "hbm" else eng.noisy_sample
                bits = sample(rec, data, shots, seed, meas, readout if ing.readout else None)
            t2 = time.perf_counter()
            counts, counts_path = _counts_of(bits, None, ing.num_clbits, ing.creg_sizes)
        t3 = time.perf_counter()
        meta = {"method": "noisy", "noisy_state": state, "noisy_measure": nmeasure, "n_qubits": width,
                "n_circuit_qubits": ing.num_qubits, "n_measure_ops": n_measure, "n_source_ops": ing.n_source_ops, "n_device_ops": len(rec),
                "n_pauli_ops": ing.n_pauli, "n_kraus_ops": ing.n_kraus, "n_kraus2_ops": ing.n_kraus2, "readout_errors": len(ing.readout), "time_compile": t1 - t0,
                "time_evolve": t2 - t1, "time_sample": t3 - t2, "time_taken": t3 - t0, "seed_simulator": seed, "counts_path": counts_path}
        meta.update(accept_meta)
        self.last_engine = None          # no resident state: every shot had its own
        self.last_plan = None
        self._last_comm = None
        return {"name": getattr(circuit, "name", "circuit"), "shots": shots, "counts": counts, "metadata": meta}

    # ---- dynamic=True: reset, classical conditions, measured qubits used again ---------------------------
    def _run_dynamic(self, circs, feats, shots, seed, opts, run_options, method, state, dmeasure):
        """the experiments of a ``run(dynamic=True)`` in which some circuit holds a reset, a condition or a gate on a measured
        qubit (``feats``: its dynamic ingest without noise).  Such a circuit runs shot by shot through ``_run_noisy`` under the
        given model or an empty one (method 'density_matrix': a circuit whose only dynamic feature is ``reset`` runs exactly,
        the reset as the record ``qsv_density_exec_accept`` documents as the reset channel); a circuit of the batch without any
        of it runs as without the option, under its own seed"""
        if opts.get("post_select") is not None:
            raise ValueError("post_select conditions the exact state vector of an ideal run; a dynamic circuit (dynamic=True: reset, "
                             "classical conditions, measured qubits used again) runs shot by shot and has none: use accept")
        if method == "trajectory":
            raise ValueError("method='trajectory' follows the outcomes of a circuit without reset and conditions; a dynamic circuit "
                             "(dynamic=True) runs shot by shot: method='statevector', or 'density_matrix' for resets alone")
        comm = opts["comm"] or SingleProcess()
        if comm.world > 1:
            raise ValueError("dynamic circuits take one process (a process group of %d ranks was given; limit 1)" % comm.world)
        if len(tuple(opts["devices"])) > 1:
            raise ValueError("dynamic circuits take one device (%d were given; limit 1)" % len(tuple(opts["devices"])))
        model = opts.get("noise_model")
        if model is not None and not isinstance(model, _noise.NoiseModel):
            raise TypeError("noise_model must be a qcmrf_amd.noise.NoiseModel, not %s" % type(model).__name__)
        model = model if model is not None else _noise.NoiseModel()
        accept = opts.get("accept")
        if accept is not None:
            if isinstance(accept, dict):
                accept = [accept] * len(circs)
            accept = list(accept)
            if len(accept) != len(circs) or not all(isinstance(d, dict) for d in accept):
                raise ValueError("accept is one {classical bit: 0 | 1} dict, or a list of %d of them (one per circuit)" % len(circs))
        exps = []
        for i, (c, f) in enumerate(zip(circs, feats)):
            extra = {"dynamic": True, "n_if_ops": f.n_if, "n_reset_ops": f.n_reset}
            if not (f.n_if or f.n_reset or f.n_reuse):
                sub = dict(run_options, dynamic=False)
                if accept is not None:
                    sub["accept"] = accept[i]
                exps.append(self.run(c, shots=shots, seed_simulator=seed + i, **sub).result().results[0])
                continue
            if f.num_clbits > 64:
                raise ValueError("dynamic circuits record at most 64 classical bits, the circuit has %d" % f.num_clbits)
            if method == "density_matrix":
                prepared, place = self._prepare_density_dynamic(c, model, accept and accept[i])
                exp = self._run_density(c, shots, seed + i, opts, prepared, accept=accept and accept[i], place=place)
                extra["n_reset_ops"] = place["n_reset"]
            else:
                prepared = self._prepare_noisy_dynamic(c, model, state)
                exp = self._run_noisy(c, shots, seed + i, opts, prepared, accept=accept and accept[i])
                extra.update(n_if_ops=prepared[0].n_if, n_reset_ops=prepared[0].n_reset)
            exp["metadata"].update(extra)
            exps.append(exp)
        return exps

    @staticmethod
    def _prepare_noisy_dynamic(circuit, model, state):
        """``_prepare_noisy_in_place`` for a dynamic circuit: the ops of ``ingest(dynamic=True)`` under the model, remapped to
        live slots by ``trajectory.plan_slots_dynamic``; every measure that is not part of the joint final draw is one
        QSV_OP_MEASURE record, every reset that stays one QSV_OP_RESET record, every guard one QSV_OP_IF record.  There is no
        deferred form, so the measurements are in place whatever noisy_measure says"""
        from . import ir, trajectory
        t0 = time.perf_counter()
        ing = _ingest.ingest(circuit, noise=model, dynamic=True)
        if ing.num_clbits > 64:
            raise ValueError("dynamic circuits record at most 64 classical bits, the circuit has %d" % ing.num_clbits)
        items, width, finals = trajectory.plan_slots_dynamic(ing.ops)
        width = max(width, 1)
        state = QsvBackend._resolve_noisy_state(state, width, " live at once with its measurements taken in place")
        early = {item[2] for item in items if isinstance(item, tuple) and item[0] == "measure"}
        late = [(s, c) for s, c in finals if c in early]    # a bit written earlier and again at the end: a record as well, so
        finals = [(s, c) for s, c in finals if c not in early]   # that the last write wins
        ops, n_measure, n_reset = [], 0, 0
        for item in items:
            if not isinstance(item, tuple):
                ops.append(item)
            elif item[0] == "measure":
                _, s, c, release, q = item
                ops.append(ir.Op("measure", target=s, mask=c, vals=(int(release),), table=model.readout_flips(q)))
                n_measure += 1
            else:
                ops.append(ir.Op("reset", target=item[1]))
                n_reset += 1
        for s, c in late:
            ops.append(ir.Op("measure", target=s, mask=c, vals=(0,), table=ing.readout.get(c)))
            n_measure += 1
        ing.ops = ops
        ing.n_reset = n_reset                                # (a trailing reset is dropped)
        clist = sorted(ing.measure)
        meas = [-1] * (clist[-1] + 1) if clist else []
        rec, data = program.encode(ops, n_meas=len(meas))
        readout = np.zeros((len(meas), 2))
        for s, c in finals:
            meas[c] = s
            readout[c] = ing.readout.get(c, (0.0, 0.0))
        return ing, rec, data, clist, meas, readout, time.perf_counter() - t0, state, ("in_place", width, n_measure)

    @staticmethod
    def _prepare_density_dynamic(circuit, model, accept):
        """(the tuple of ``_prepare_density``, place) for a dynamic circuit under method 'density_matrix': resets only.  A reset
        becomes the MEASURE record with release = 1 whose classical bit no ``fix_mask`` holds (``qsv_density_exec_accept``: the
        reset channel), the plan is ``trajectory.plan_slots_dynamic``; a mid-circuit measure follows the rule of
        ``density_measure='in_place'`` (fixed by ``accept`` and written once).  Conditions, and a measured qubit used again
        without a reset in between, would need branching and are refused"""
        from . import ir, trajectory
        t0 = time.perf_counter()
        ing = _ingest.ingest(circuit, noise=model, dynamic=True)
        if ing.n_if:
            raise ValueError("method='density_matrix' runs the resets of a dynamic circuit, not its classical conditions (%d here): a "
                             "density matrix cannot follow a measured bit without branching; run it shot by shot "
                             "(method='statevector', dynamic=True)" % ing.n_if)
        if ing.n_reuse:
            raise ValueError("method='density_matrix': a measured qubit is used again without a reset in between (%d times); a density "
                             "matrix cannot follow the measured bit without branching; run it shot by shot (method='statevector', "
                             "dynamic=True)" % ing.n_reuse)
        items, width, finals = trajectory.plan_slots_dynamic(ing.ops)
        width = max(width, 1)
        if width > _lib.DENSITY_MAX_QUBITS:
            raise ValueError("method='density_matrix' holds rho of at most %d qubits (16 * 4^W bytes), the circuit has %d live at once "
                             "with its measurements taken in place" % (_lib.DENSITY_MAX_QUBITS, width))
        early = [item for item in items if isinstance(item, tuple) and item[0] == "measure"]
        written = {}
        for c in [item[2] for item in early] + [c for _, c in finals]:
            written[c] = written.get(c, 0) + 1
        for _, s, c, release, q in early:
            if accept is not None and c in accept and accept[c] not in (0, 1):
                raise ValueError("accept fixes classical bit %r to %r; a bit reads 0 or 1" % (c, accept[c]))
            if accept is not None and c in accept and written[c] == 1:
                continue
            why = "is written %d times" % written[c] if accept is not None and c in accept else "is not fixed by accept"
            raise ValueError("method='density_matrix', dynamic=True: classical bit %d is measured mid-circuit (qubit %d) and %s; a "
                             "density matrix follows a measurement taken in place only where its outcome is fixed and written "
                             "once: pass accept={%d: 0 or 1}" % (c, q, why, c))
        final = dict((c, s) for s, c in finals)
        clist = sorted(final)
        if len(clist) > DENSITY_MAX_CLBITS:
            raise ValueError("method='density_matrix' returns the distribution over at most %d written classical bits, the "
                             "circuit's trailing measurements write %d" % (DENSITY_MAX_CLBITS, len(clist)))
        every = sorted(ing.measure)
        if every and every[-1] >= 64:
            raise ValueError("method='density_matrix' records at most 64 classical bits, the circuit writes bit %d" % every[-1])
        fm = fv = n_reset = 0
        for _, s, c, release, q in early:
            fm |= 1 << int(c)
            fv |= int(accept[c]) << int(c)
        free_bit = next((b for b in range(64) if not (fm >> b) & 1), None)
        if free_bit is None and any(isinstance(item, tuple) and item[0] == "reset" for item in items):
            raise ValueError("method='density_matrix': accept fixes all 64 classical bits, a reset needs one that is not fixed")
        ops = []
        for item in items:
            if not isinstance(item, tuple):
                ops.append(item)
            elif item[0] == "measure":
                _, s, c, release, q = item
                ops.append(ir.Op("measure", target=s, mask=c, vals=(int(release),), table=model.readout_flips(q)))
            else:                                            # the reset channel: outcome forgotten, the 1 half moved to 0
                ops.append(ir.Op("measure", target=item[1], mask=free_bit, vals=(1,), table=None))
                n_reset += 1
        ing.ops = ops
        rec, data = program.encode(ops)
        meas = [-1] * (every[-1] + 1) if every else []
        readout = np.zeros((len(meas), 2))
        for c in clist:
            meas[c] = final[c]
            readout[c] = ing.readout.get(c, (0.0, 0.0))
        place = {"mode": "in_place", "width": width, "n_measure": len(early), "fix": (fm, fv), "n_reset": n_reset}
        return (ing, rec, data, clist, meas, readout, time.perf_counter() - t0), place

    # ---- method="density_matrix": rho of W qubits in a vector of 2W ---------------------------------
    @staticmethod
    def _density_model_of(opts):
        """the model of a density-matrix run: the given one, or an empty one (no model, the ideal distribution)"""
        model = opts.get("noise_model")
        if model is not None and not isinstance(model, _noise.NoiseModel):
            raise TypeError("noise_model must be a qcmrf_amd.noise.NoiseModel, not %s" % type(model).__name__)
        comm = opts["comm"] or SingleProcess()
        if comm.world > 1:
            raise ValueError("method='density_matrix' takes one process (a process group of %d ranks was given; limit 1)" % comm.world)
        return model if model is not None else _noise.NoiseModel()

    @staticmethod
    def _prepare_density(circuit, model):
        """host half of a density-matrix run: the record stream of a noisy run (ingest with the model + encode)"""
        t0 = time.perf_counter()
        ing = _ingest.ingest(circuit, noise=model)
        if ing.num_qubits > _lib.DENSITY_MAX_QUBITS:
            raise ValueError("method='density_matrix' holds rho of at most %d qubits (16 * 4^W bytes), the circuit has %d"
                             % (_lib.DENSITY_MAX_QUBITS, ing.num_qubits))
        clist = sorted(ing.measure)
        if len(clist) > DENSITY_MAX_CLBITS:
            raise ValueError("method='density_matrix' returns the distribution over at most %d written classical bits, the "
                             "circuit writes %d" % (DENSITY_MAX_CLBITS, len(clist)))
        if clist and clist[-1] >= 64:
            raise ValueError("method='density_matrix' records at most 64 classical bits, the circuit writes bit %d" % clist[-1])
        rec, data = program.encode(ing.ops)
        meas = [-1] * (clist[-1] + 1) if clist else []
        readout = np.zeros((len(meas), 2))
        for c in clist:
            meas[c] = ing.measure[c]
            readout[c] = ing.readout.get(c, (0.0, 0.0))
        return ing, rec, data, clist, meas, readout, time.perf_counter() - t0

    @staticmethod
    def _prepare_density_measure(circuit, model, measure, accept):
        """(the tuple of ``_prepare_density``, place) for the run option density_measure: ``place`` is None for the default
        (``measure`` None or 'deferred': today's path and metadata), else {"mode": the option resolved, ...}"""
        if measure is None or measure == "deferred":
            return QsvBackend._prepare_density(circuit, model), None
        t0 = time.perf_counter()
        got = QsvBackend._prepare_density_in_place(circuit, model, accept, measure == "auto", t0)
        if got is not None:
            return got
        prepared = QsvBackend._prepare_density(circuit, model)
        return prepared, {"mode": "deferred", "width": prepared[0].num_qubits, "n_measure": 0}

    @staticmethod
    def _prepare_density_in_place(circuit, model, accept, auto, t0):
        """``_prepare_density`` with the mid-circuit measurements applied where they occur: the ops of the deferred ingest in
        their order, remapped to live slots (``trajectory.plan_slots``), every mid-circuit measure a "measure" op built as
        ``_prepare_noisy_in_place`` builds it (one QSV_OP_MEASURE record, its flips those of the measured logical qubit); the
        trailing measures stay the read-out of the diagonal (``clist``, ``meas`` and ``readout`` cover them alone).  rho
        cannot follow a bit that is free, so every mid-circuit bit has to be fixed by ``accept`` and written once: otherwise
        a ValueError, or None under ``auto``, which also answers None when the live width is the circuit's"""
        from . import ir, trajectory
        ing = _ingest.ingest(circuit, noise=model, keep_measures=True)
        staged, width, finals = trajectory.plan_slots(ing.ops)
        width = max(width, 1)
        if auto and width >= ing.num_qubits:
            return None
        early = [item for item in staged if item[0] == "measure"]
        written = {}
        for c in [item[2] for item in early] + [c for _, c in finals]:
            written[c] = written.get(c, 0) + 1
        for _, s, c, release, q in early:
            if accept is not None and c in accept and accept[c] not in (0, 1):
                raise ValueError("accept fixes classical bit %r to %r; a bit reads 0 or 1" % (c, accept[c]))
            if accept is not None and c in accept and written[c] == 1:
                continue
            if auto:
                return None
            why = "is written %d times" % written[c] if accept is not None and c in accept else "is not fixed by accept"
            raise ValueError("density_measure='in_place': classical bit %d is measured mid-circuit (qubit %d) and %s; a density matrix "
                             "follows a measurement taken in place only where its outcome is fixed and written once: pass "
                             "accept=qc.post_selection(), or density_measure='deferred' or 'auto'" % (c, q, why))
        if width > _lib.DENSITY_MAX_QUBITS:
            raise ValueError("method='density_matrix' holds rho of at most %d qubits (16 * 4^W bytes), the circuit has %d live at once "
                             "with its measurements taken in place" % (_lib.DENSITY_MAX_QUBITS, width))
        final = dict((c, s) for s, c in finals)             # (a bit two trailing measures write: the last one reads it)
        clist = sorted(final)
        if len(clist) > DENSITY_MAX_CLBITS:
            raise ValueError("method='density_matrix' returns the distribution over at most %d written classical bits, the "
                             "circuit's trailing measurements write %d" % (DENSITY_MAX_CLBITS, len(clist)))
        every = sorted(ing.measure)
        if every and every[-1] >= 64:
            raise ValueError("method='density_matrix' records at most 64 classical bits, the circuit writes bit %d" % every[-1])
        ops, fm, fv = [], 0, 0
        for item in staged:
            if item[0] == "ops":
                ops += item[1]
            else:
                _, s, c, release, q = item
                ops.append(ir.Op("measure", target=s, mask=c, vals=(int(release),), table=model.readout_flips(q)))
                fm |= 1 << int(c)
                fv |= int(accept[c]) << int(c)
        ing.ops = ops
        rec, data = program.encode(ops)
        meas = [-1] * (every[-1] + 1) if every else []
        readout = np.zeros((len(meas), 2))
        for c in clist:
            meas[c] = final[c]
            readout[c] = ing.readout.get(c, (0.0, 0.0))
        place = {"mode": "in_place", "width": width, "n_measure": len(early), "fix": (fm, fv)}
        return (ing, rec, data, clist, meas, readout, time.perf_counter() - t0), place

    @staticmethod
    def _confuse(dist, flips):
        """readout confusion on the host: bit j of the index flipped with flips[j][value]"""
        words = np.arange(dist.size)
        for j, (f0, f1) in enumerate(flips):
            if f0 == 0.0 and f1 == 0.0:
                continue
            go = np.where((words >> j) & 1, f1, f0)
            new = dist * (1.0 - go)
            new[words ^ (1 << j)] += dist * go
            dist = new
        return dist

    @staticmethod
    def _condition(dist, clist, accept, total=None):
        """(dist conditioned on ``accept`` and renormalised, the mass of the condition); index bit j of dist is classical bit
        clist[j].  ``total``: what the mass is a share of (default: the sum of dist)"""
        fm = fv = 0
        for c, v in accept.items():
            if c not in clist:
                raise ValueError("accept names classical bit %r, which no measurement writes" % (c,))
            if v not in (0, 1):
                raise ValueError("accept fixes classical bit %r to %r; a bit reads 0 or 1" % (c, v))
            fm |= 1 << clist.index(c)
            fv |= int(v) << clist.index(c)
        p = np.clip(dist, 0.0, None)
        kept = np.where((np.arange(p.size) & fm) == fv, p, 0.0)
        mass = kept.sum()
        if not mass > 0:
            raise ValueError("post-selected outcome %r has zero probability" % (accept,))
        return kept / mass, float(mass / (p.sum() if total is None else total))

    def _run_density(self, circuit, shots, seed, opts, prepared, accept=None, place=None):
        """qsv_density_exec, then the exact distribution (qsv_density_diagonal + readout confusion) and the shots (qsv_density_sample);
        ``accept``: the distribution conditioned on the host, the shots one multinomial draw from it.
        ``place`` (``_prepare_density_measure``) in place: qsv_density_exec_accept with the accepted bits its MEASURE records
        write -- rho comes back with their share of the success probability as its trace --, the diagonal over the slots of
        the trailing measurements, the accepted bits among those conditioned on the host"""
        ing, rec, data, clist, meas, readout, t_compile = prepared
        t1 = time.perf_counter()
        t0 = t1 - t_compile
        in_place = place is not None and place["mode"] == "in_place"
        W = place["width"] if in_place else ing.num_qubits
        if in_place and accept is not None:
            self._accept_mask(accept, ing)                     # (its refusals: a bit nothing writes, a value that is no bit)
        state_bytes = 16 * 4 ** W
        dev = tuple(opts["devices"])[0]
        memory = _lib.device_memory if self._engine_factory is None else getattr(self._engine_factory, "device_memory", None)
        if memory is not None and not (self._engine is not None and self._engine_key == (2 * W, (dev,))):
            free = memory(dev)[0]
            if state_bytes > free:
                raise ValueError("method='density_matrix': rho of %d qubits takes 16 * 4^%d = %d bytes, device %d has %d free"
                                 % (W, W, state_bytes, dev, free))
        eng = self._get_engine(2 * W, dict(opts, comm=None, devices=tuple(opts["devices"])[:1]))
        self._apply_engine_options(eng, opts)
        if in_place:
            eng.density_exec_accept(rec, data, *place["fix"])
        else:
            eng.density_exec(rec, data)
        eng.sync()
        t2 = time.perf_counter()
        marg, trace = eng.density_diagonal([meas[c] if in_place else ing.measure[c] for c in clist])
        dist = self._confuse(marg, [tuple(readout[c]) for c in clist])
        accept_meta = {}
        if accept is not None and in_place:
            # the records' share is in the trace already: the mass of the matching words is the whole success probability
            dist, mass = self._condition(dist, clist, {c: v for c, v in accept.items() if not (place["fix"][0] >> int(c)) & 1}, total=1.0)
            accept_meta = {"accept": dict(accept), "accept_probability": mass}
        elif accept is not None:
            dist, mass = self._condition(dist, clist, accept)
            accept_meta = {"accept": dict(accept), "accept_probability": mass}
        keep = np.flatnonzero(dist > 0)
        words = np.zeros(keep.size, dtype=np.uint64)            # bit j of the index is classical bit clist[j]
        for j, c in enumerate(clist):
            words |= ((keep.astype(np.uint64) >> np.uint64(j)) & np.uint64(1)) << np.uint64(c)
        if in_place:
            words |= np.uint64(place["fix"][1])                 # full-width keys: the bits the records wrote read their accepted values
        probs = dict(zip(_format_keys(words, np.arange(keep.size), ing.num_clbits, ing.creg_sizes).keys(), dist[keep].tolist())) if clist or (in_place and place["n_measure"]) else {}
        counts = {}
        counts_path = _counts_path_default()
        if (clist or (in_place and place["n_measure"])) and shots > 0 and accept is not None:
            drawn = np.random.default_rng(seed).multinomial(shots, dist[keep])
            counts = _format_keys(words[drawn > 0], drawn[drawn > 0], ing.num_clbits, ing.creg_sizes)
            counts_path = "python"
        elif clist and shots > 0:
            bits = eng.density_sample(shots, seed, meas, readout if ing.readout else None)
            counts, counts_path = _counts_of(bits, None, ing.num_clbits, ing.creg_sizes)
        t3 = time.perf_counter()
        meta = {"method": "density_matrix", "n_qubits": W, "n_source_ops": ing.n_source_ops, "n_device_ops": len(rec),
                "n_pauli_ops": ing.n_pauli, "n_kraus_ops": ing.n_kraus, "n_kraus2_ops": ing.n_kraus2, "readout_errors": len(ing.readout), "trace": float(trace),
                "state_bytes": state_bytes, "time_compile": t1 - t0, "time_evolve": t2 - t1, "time_sample": t3 - t2,
                "time_taken": t3 - t0, "seed_simulator": seed, "counts_path": counts_path}
        if place is not None:
            meta.update(density_measure=place["mode"], n_circuit_qubits=ing.num_qubits, n_measure_ops=place["n_measure"])
        meta.update(accept_meta)
        self.last_engine = None          # the resident vector is rho, not a state: statevector() has nothing to show
        self.last_plan = None
        self._last_comm = None
        return {"name": getattr(circuit, "name", "circuit"), "shots": shots, "counts": counts, "probabilities": probs,
                "metadata": meta}

    def _apply_engine_options(self, eng, opts):
        """engine options are per RUN: whatever an earlier call set on the cached engine and this one does not ask for
        goes back to the library default first"""
        want = dict(opts["engine_options"] or {})
        applied = getattr(eng, "_applied_options", None)
        if applied is None:
            applied = eng._applied_options = {}
        for k in [k for k in applied if k not in want]:
            if k in _lib.OPTION_DEFAULTS:
                eng.set_option(k, _lib.OPTION_DEFAULTS[k])
            del applied[k]
        for k, v in want.items():
            eng.set_option(k, v)
            applied[k] = v

    def _prepare(self, circuit, opts):
        """host half of a run: ingest + passes + plan + encode (no device work).  A circuit of the reference's construction is
        compiled by the native front end instead of ingest + passes where that applies (``frontend.compile_blocks``; the
        same program): ``compile_path`` "blocks", else "passes".  Such a circuit is also planned and encoded in native code
        where that applies (``frontend.build_program``; the same records): ``plan_path`` "native", else "python"."""
        t0 = time.perf_counter()
        comm = opts["comm"] or SingleProcess()
        n_shards = comm.world if comm.world > 1 else len(opts["devices"])
        spmd = comm.world > 1 and opts.get("spmd_ingest", False) and not opts.get("_batch")
        copts = {k: opts[k] for k in ("fusion", "layout", "engine_options", "fold_fresh")}
        front = None
        if (copts["fusion"] == 3 and copts["fold_fresh"] and not spmd and not opts.get("dynamic")
                and opts.get("method", "statevector") == "statevector"):
            g = max(1, int(n_shards)).bit_length() - 1
            front = frontend.front_half(circuit, max(1, min(5, int(circuit.num_qubits) - g)))
        if front is not None:
            ing = front[0]
            ing.compile_path = "blocks"
            done = frontend.build_program(front, n_shards, copts["layout"])
            if done is not None:
                ing.plan_path = "native"
                return (ing,) + done + (n_shards, time.perf_counter() - t0)
            pl = self._plan(ing, frontend.fold_ops(*front[1:]), n_shards, dict(self.options, **copts))
        else:
            ing, pl = self.compile(circuit, n_shards, ingest_comm=comm if spmd else None, **copts)
        rec, data = program.encode(pl.ops)
        return ing, pl, rec, data, n_shards, time.perf_counter() - t0

    def compile(self, circuit, n_shards=1, **options):
        """ingest + passes + plan only (no GPU): returns (Ingested, Plan)"""
        opts = dict(self.options)
        opts.update(options)
        ing = _ingest.ingest(circuit, peephole=opts["fusion"] >= 1, comm=opts.get("ingest_comm"), compact=opts["fusion"] >= 3)
        # every qubit of a dense window has to be local to a shard at the same time
        g = max(1, int(n_shards)).bit_length() - 1
        ops = passes.optimise(ing.ops, level=opts["fusion"], fresh=bool(opts.get("fold_fresh", True)),
                              dense_kmax=max(1, min(5, ing.num_qubits - g)), flat=ing.flat)
        return ing, self._plan(ing, ops, n_shards, opts)

    @staticmethod
    def _plan(ing, ops, n_shards, opts):
        """the fused ops with the circuit's global phase put in, planned onto the shards"""
        if ing.global_phase and opts.get("apply_global_phase", True):
            from . import ir
            ph = np.exp(1j * ing.global_phase)
            host = next((o for o in ops if o.kind == "diag"), None)
            if host is not None:                             # rides in a diagonal that is there anyway (one factor fewer on the device)
                host.table = host.table * ph
            else:
                ops.append(ir.op_diag([0], [ph, ph]))
        eo = opts.get("engine_options") or {}
        lane = bool(eo.get("lane_targets", 1)) and not eo.get("zero_tracking", 0)   # lane targets need a fully populated vector
        return planner.plan(ops, ing.num_qubits, n_shards, opts["layout"], lane_targets=lane,
                            dyn_lanes=int(eo.get("dyn_lanes", planner.DYN_LANES)))

    def _run_trajectory(self, circuit, shots, seed, opts):
        from . import trajectory
        t0 = time.perf_counter()
        vals, cnts, num_clbits, creg_sizes, meta = trajectory.run_trajectories(
            circuit, shots, seed, fusion=opts["fusion"], device=tuple(opts["devices"])[0],
            engine_factory=self._engine_factory, walk=opts.get("trajectory_walk") or "depth",
            slots=opts.get("trajectory_slots"), trace=opts.get("trajectory_trace"))
        agg = {}
        for v, c in zip(vals.tolist(), cnts.tolist()):
            agg[v] = agg.get(v, 0) + c
        if vals.dtype == object:
            uv = np.empty(len(agg), dtype=object)
            uv[:] = list(agg.keys())
        else:
            uv = np.fromiter(agg.keys(), dtype=np.uint64, count=len(agg))
        uc = np.fromiter(agg.values(), dtype=np.int64, count=len(agg))
        counts = _format_keys(uv, uc, num_clbits, creg_sizes) if len(agg) else {}
        meta.update({"n_qubits": int(circuit.num_qubits), "time_taken": time.perf_counter() - t0,
                     "time_sample": 0.0, "seed_simulator": seed, "fusion": opts["fusion"]})
        return {"name": getattr(circuit, "name", "circuit"), "shots": shots, "counts": counts, "metadata": meta}

    @staticmethod
    def _to_clbits(bits, clist, direct):
        """sampled words -> classical-register values (bit c = classical bit c)"""
        if direct:
            return bits
        vals = np.zeros(bits.shape, dtype=np.uint64)
        for j, c in enumerate(clist):
            vals |= ((bits >> np.uint64(j)) & np.uint64(1)) << np.uint64(c)
        return vals

    def _run_one(self, circuit, shots, seed, opts, prepared=None, post_select=None):
        if opts.get("method", "statevector") == "trajectory":
            return self._run_trajectory(circuit, shots, seed, opts)
        comm = opts["comm"] or SingleProcess()
        ing, pl, rec, data, n_shards, t_compile = prepared if prepared is not None else self._prepare(circuit, opts)
        t1 = time.perf_counter()
        t0 = t1 - t_compile

        fix = None if post_select is None else self._post_select_mask(post_select, ing, pl)
        eng = self._get_engine(ing.num_qubits, opts)
        self._apply_engine_options(eng, opts)      # (the plan above was compiled for exactly this call's options)
        if (shots <= 0 or not ing.measure) and fix is None and "defer_state" not in (opts["engine_options"] or {}):
            # nothing will be sampled, so the caller is after the state: have the generator write it at once instead of
            # leaving tile sums first and writing it on the first read (the next run's options undo this)
            eng.set_option("defer_state", 0)
            eng._applied_options["defer_state"] = 0
        if pl.n_exchanges and not eng._comm_ready:
            # collective: RCCL communicator over all ranks, or peer-mapped shards (ranks sharing a GPU)
            eng.comm_bootstrap(comm, device=opts["device"], transport=opts.get("exchange", "auto"))
            eng._comm_ready = True
        if opts["profile"]:
            eng.set_profiling(True)
        eng.reset_stats()
        eng.exec(rec, data)
        eng.sync()
        t2 = time.perf_counter()

        clist = sorted(ing.measure)
        # output bit c <- the qubit measured into classical bit c (-1: never written, stays 0), so
        # the sampled words come back already laid out as the classical register
        if clist and clist[-1] < 64:
            meas_phys = [-1] * (clist[-1] + 1)
            for c in clist:
                meas_phys[c] = pl.layout[ing.measure[c]]
            direct = True
        else:
            meas_phys = [pl.layout[ing.measure[c]] for c in clist]
            direct = False
        counts = {}
        counts_path = _counts_path_default()
        post_meta = {}
        # the words are only counted here: the draws without the shuffle (qsv_sample_unordered, the same multiset); an engine
        # that has only the ordered calls is asked for those
        draw = getattr(eng, "sample_unordered", None) or eng.sample
        if fix is not None:
            # every shot from the state conditioned on the fixed bits (qsv_sample_cond): the words keep their full width,
            # the fixed bits reading their values; the mass of the condition over the norm is its exact probability
            draw_cond = getattr(eng, "sample_cond_unordered", None) or eng.sample_cond
            before = eng.state_info()
            words, mass = draw_cond(max(shots, 0) if clist else 0, seed, meas_phys, fix[0], fix[1])
            after = eng.state_info()
            if not mass > 0:
                raise ValueError("post-selected outcome %r has zero probability" % (post_select,))
            if clist and shots > 0:
                counts, counts_path = _counts_of(self._to_clbits(words, clist, direct), None, ing.num_clbits, ing.creg_sizes)
            post_meta = {"post_select": dict(post_select), "post_select_probability": mass / eng.norm(),
                         "post_select_path": "stored" if not before["deferred"] else
                                             "realized" if after["realize_calls"] > before["realize_calls"] else "listed"}
        elif clist and shots > 0:
            if comm.world > 1:
                # One round trip and one one-way send per run: (1) all-gather of one double per rank, the shard's
                # probability mass -> the common multinomial split of the shots over the shards (same seed on every
                # rank); (2) each rank draws exactly split[rank] outcomes from its own shard and SENDS them to rank 0
                # as (distinct outcome, count) pairs -- a few hundred pairs -- without waiting for anything back.
                # Only rank 0 merges and formats: Result.get_counts() is the merged dict there and empty on the
                # other ranks (metadata "counts_on_rank": 0), whose step ends with the send -- formatting 4096 keys on
                # every rank was host time that does not shrink with the rank count (``gather_counts="all"``
                # restores the all-gather: every rank then returns the full dict).
                masses = np.asarray(comm.allgather_f64(eng.norm()) if hasattr(comm, "allgather_f64")
                                    else comm.allgather(eng.norm()), dtype=np.float64)
                split = np.random.RandomState(seed % (2 ** 32)).multinomial(shots, masses / masses.sum())
                k = int(split[comm.rank])
                mine = draw(k, (seed * 1315423911 + comm.rank) % (2 ** 63), meas_phys) if k else np.zeros(0, dtype=np.uint64)
                uv, uc = np.unique(self._to_clbits(mine, clist, direct), return_counts=True)
                pairs = np.concatenate([uv, uc.astype(np.uint64)])
                everyone = opts.get("gather_counts", "root") == "all"
                if everyone or not hasattr(comm, "gather_bytes"):
                    raw = comm.allgather_bytes(pairs.tobytes()) if hasattr(comm, "allgather_bytes") else [np.asarray(b, dtype=np.uint64).tobytes() for b in comm.allgather(pairs)]
                else:
                    raw = comm.gather_bytes(pairs.tobytes())
                if raw is not None:
                    parts = [np.frombuffer(b, dtype=np.uint64) for b in raw]
                    av = np.concatenate([b[:b.size // 2] for b in parts])
                    ac = np.concatenate([b[b.size // 2:] for b in parts]).astype(np.int64)
                    # shards that differ only in an unmeasured qubit can produce the same outcome: their counts are summed
                    counts, counts_path = _counts_of(av, ac, ing.num_clbits, ing.creg_sizes)
            else:
                vals = self._to_clbits(draw(shots, seed, meas_phys), clist, direct)
                counts, counts_path = _counts_of(vals, None, ing.num_clbits, ing.creg_sizes)
        elif shots > 0:
            counts = {}
        t3 = time.perf_counter()
        meta = {"n_qubits": ing.num_qubits, "n_source_ops": ing.n_source_ops, "n_device_ops": len(pl.ops),
                "n_exchanges": pl.n_exchanges, "n_shards": n_shards, "layout": list(pl.layout),
                "fusion": opts["fusion"], "time_compile": t1 - t0, "time_evolve": t2 - t1,
                "time_sample": t3 - t2, "time_taken": t3 - t0, "seed_simulator": seed, "ingest_path": ing.ingest_path,
                "compile_path": ing.compile_path, "plan_path": ing.plan_path, "counts_path": counts_path}
        meta.update(post_meta)
        if comm.world > 1 and opts.get("gather_counts", "root") != "all":
            meta["counts_on_rank"] = 0
        if opts["profile"]:
            meta["stats"] = eng.stats()
            eng.set_profiling(False)
        self.last_engine = eng
        self.last_plan = pl
        self._last_comm = comm
        return {"name": getattr(circuit, "name", "circuit"), "shots": shots, "counts": counts, "metadata": meta}


class _Provider:
    """``from qcmrf_amd import Aer`` -> ``Aer.get_backend('qasm_simulator')`` (run_experiment.py:14,54)."""

    def __init__(self):
        self._cache = {}

    def get_backend(self, name="qasm_simulator", **options):
        if name not in _NAMES:
            raise ValueError("unknown backend %r; this provider serves %s" % (name, ", ".join(_NAMES)))
        if options or name not in self._cache:
            b = QsvBackend(name, **options)
            if options:
                return b
            self._cache[name] = b
        return self._cache[name]

    def backends(self):
        return list(_NAMES)


Aer = _Provider()


def get_backend(name="qasm_simulator", **options):
    return Aer.get_backend(name, **options)
