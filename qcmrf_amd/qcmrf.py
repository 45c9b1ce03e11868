"""``QCMRF(cliques, theta, ...)`` -- the reference's circuit model behind the same constructor.

Mirrors the public surface of /root/reference/QCMRF.py:13-157,199-284 (constructor signature,
properties, ValueError texts, gate order, default-theta RNG draws, post-processing helpers) so
that ``run_experiment.py`` style scripts run unchanged.  When Qiskit is importable the class
derives from the real ``qiskit.QuantumCircuit`` (and uses the real ``AND``); otherwise from the
container in ``qcmrf_amd.circuit``.  Either way the object is what the engine's ingest reads.

``sufficient_statistic`` / ``Hamiltonian`` (QCMRF.py:159-197) exist here as the diagonals they are
(``hamiltonian_diagonal``, ``sufficient_statistic_diagonal``: opflow was removed from Qiskit), with
their expectation values evaluated on the device (``expectation_hamiltonian``,
``expectation_sufficient_statistic`` -> libqsv ``qsv_expect_diag``).
"""
from __future__ import annotations

import itertools

import numpy as np

from . import mrf

try:                                             # pragma: no cover - Qiskit absent in this image
    from qiskit import QuantumCircuit
    from qiskit.circuit.library import AND
    HAVE_QISKIT = True
except Exception:                                # ModuleNotFoundError here
    from .circuit import QuantumCircuit, AND
    HAVE_QISKIT = False

DEFAULT_BASIS = ['cx', 'id', 'rz', 'sx', 'x']


class QCMRF(QuantumCircuit):
    """Quantum circuit Markov random field (Gibbs-state preparation by real-part extraction)."""

    def __init__(self, cliques=None, theta=None, gamma=None, beta: float = 1, name: str = "QCMRF",
                 with_measurements=True, with_barriers=False, basis_gates=DEFAULT_BASIS):
        self._cliques, self._theta, self._gamma = cliques, theta, gamma
        self._beta, self._name = beta, name
        self._with_measurements, self._with_barriers = with_measurements, with_barriers
        self.basis_gates = basis_gates

        # same acceptance test and message as QCMRF.py:45-48 (only the first element is inspected)
        ok = type(cliques) == list and type(cliques[0]) == list and type(cliques[0][0]) == int
        if not ok:
            raise ValueError("The set of clique is not set properly. Type must be list of list of int.")

        self._num_cliques = len(cliques)
        self._n = max(cliques[0][0], max(v for C in cliques for v in C)) + 1      # QCMRF.py:52-57
        sizes = [len(C) for C in cliques]
        self._dim = sum(2 ** k for k in sizes)                                     # QCMRF.py:59-65
        self._c_max = max([0] + sizes)

        if theta is not None and len(theta) != self._dim:                          # QCMRF.py:68-71
            raise ValueError("The parameter vector has an incorrect dimension. Expected: " + str(self._dim))
        if gamma is not None and len(gamma) != self._dim:                          # QCMRF.py:73-76
            raise ValueError("The QCMRF parameter vector has an incorrect dimension. Expected: " + str(self._dim))

        width = self._n + self._num_cliques + 1                                    # QCMRF.py:78
        super().__init__(width, width, name=name)
        self._build()

    # ---- read-only model facts (QCMRF.py:82-127) ------------------------------------------
    @property
    def dimension(self):
        """Number of parameters, sum over cliques of 2^|C|."""
        return self._dim

    @property
    def cliques(self):
        return self._cliques

    @property
    def num_vertices(self):
        return self._n

    num_nodes = num_vertices

    @property
    def num_cliques(self):
        return self._num_cliques

    @property
    def max_clique(self):
        return self._c_max

    # ---- parameters: lazily converted both ways (QCMRF.py:129-157) --------------------------
    @property
    def theta(self):
        if self._theta is None:
            self._theta = [2 * np.log(np.cos(2 * g)) / self._beta for g in self._gamma]
        return self._theta

    @property
    def gamma(self):
        if self._gamma is None:
            self._gamma = [0.5 * np.arccos(np.exp(self._beta * 0.5 * w)) for w in self._theta]
        return self._gamma

    def hamiltonian_diagonal(self):
        """H = -sum theta_{C,y} Phi_{C,y} is diagonal: H[x] = -sum_C theta_{C,x_C}; index has
        variable v on bit n-1-v (QCMRF.py:159-193 restated without opflow)."""
        n = self._n
        idx = np.arange(2 ** n)
        H = np.zeros(2 ** n)
        off = 0
        th = np.asarray(self.theta, dtype=np.float64)
        for C in self._cliques:
            y = np.zeros_like(idx)
            for j, v in enumerate(C):
                y |= ((idx >> (n - 1 - v)) & 1) << (len(C) - 1 - j)
            H -= th[off + y]
            off += 2 ** len(C)
        return H

    def sufficient_statistic_diagonal(self, C, y):
        """Phi_{C,y} = prod_{v in C} |y_v><y_v| is a diagonal projector: returns its 0/1 diagonal
        over the 2^n variable states (QCMRF.py:159-179 restated without opflow; same index
        convention as ``hamiltonian_diagonal``)."""
        n = self._n
        idx = np.arange(2 ** n)
        d = np.ones(2 ** n)
        for v, b in zip(C, y):
            d *= (((idx >> (n - 1 - v)) & 1) == int(bool(b)))
        return d

    def expectation_hamiltonian(self, backend, post_selected=True, **run_options):
        """<H> of ``Hamiltonian()`` (QCMRF.py:181-193) in the state this circuit prepares, evaluated on
        the device: the circuit is run on ``backend`` (no shots) and the diagonal H is averaged over
        the resident amplitudes in one read pass.  post_selected=True: in the state conditioned on
        every ancilla (and the AND scratch qubit) reading 0 -- the Gibbs state the construction
        targets.  Returns (<H>, probability of that condition)."""
        backend.run(self, shots=0, **run_options)
        n, W = self._n, self._n + self._num_cliques + 1
        fixed = {q: 0 for q in range(n, W)} if post_selected else None
        s0, s1 = backend.expectation_diagonal(self.hamiltonian_diagonal(), list(range(n)), fixed)
        return s0 / s1, s1

    def expectation_sufficient_statistic(self, backend, C, y, post_selected=True, **run_options):
        """<Phi_{C,y}> of ``sufficient_statistic(C, y)`` (QCMRF.py:159-179): the probability that the
        variables of C read y, same conventions as ``expectation_hamiltonian``"""
        backend.run(self, shots=0, **run_options)
        n, W = self._n, self._n + self._num_cliques + 1
        fixed = {q: 0 for q in range(n, W)} if post_selected else None
        # Phi only looks at the clique's own qubits: variable v lives on qubit n-1-v (QCMRF.py:219)
        qs = [n - 1 - v for v in C]
        tab = np.zeros(2 ** len(qs))
        tab[sum(int(bool(b)) << e for e, b in enumerate(y))] = 1.0
        s0, s1 = backend.expectation_diagonal(tab, qs, fixed)
        return s0 / s1, s1

    def marginals(self, backend, post_selected=True, circuit=None, **run_options):
        """All clique marginals of the state this circuit prepares from ONE run and one conditioned device pass:
        ``(mu, p_success)`` with ``mu[offset(C) + y] = P(x_C = y)``, a float64 vector of length ``dimension`` in the order
        of ``theta`` (clique by clique, y as ``itertools.product([0, 1], repeat=len(C))`` counts, the first variable of C
        most significant).  post_selected=True: in the state conditioned on every ancilla and the AND scratch qubit
        reading 0 -- the Gibbs state -- and ``p_success`` is the probability of that condition; only the matching
        amplitudes are read, and a state the engine left deferred stays deferred where the condition selects tiles.
        post_selected=False: the marginals of the whole state (``p_success`` 1).  With the data marginals mu-hat,
        beta (mu-hat - mu) is the gradient of the log-likelihood (``qcmrf_amd.learn``).  ``circuit``: a lowering of this
        circuit (``transpile``) to run in its place."""
        n, W = self._n, self._n + self._num_cliques + 1
        run = self if circuit is None else circuit
        if self._with_measurements and post_selected:
            # a run that conditions leaves a deferrable state deferred (a plain run without shots has it written at once)
            backend.run(run, shots=0, post_select=self.post_selection(), **run_options)
        else:
            backend.run(run, shots=0, **run_options)
        fixed = {q: 0 for q in range(n, W)} if post_selected else None
        # bin bit b <-> group[b]: the LAST variable of C on bit 0 makes the first one most significant
        groups = [[n - 1 - v for v in reversed(C)] for C in self._cliques]
        parts, mass = backend.marginals(groups, fixed)
        norm = backend.last_engine.norm()
        if not mass > 0:
            raise ValueError("the post-selected outcome has zero probability")
        return np.concatenate([np.asarray(p, dtype=np.float64) for p in parts]) / mass, mass / norm

    def conditional_marginals(self, backend, rows, circuit=None, **run_options):
        """The clique marginals of the Gibbs state given every data row's observed values, from ONE run and ONE batched
        device pass: ``(mu, p_rows, p_success)``.  ``rows`` is an int array (B, n), rows[r, v] the value of variable v or
        -1 where it is unobserved; ``mu[r]`` is ``marginals`` of the state conditioned on row r's evidence (length
        ``dimension``, the order of ``theta``), ``p_rows[r]`` is P(observed part of row r) under the Gibbs distribution
        and ``p_success`` the probability that every ancilla and the AND scratch qubit read 0.  Every row fixes those
        qubits to 0 and its observed variables (variable v on qubit n-1-v); one more condition fixes the ancillas
        alone, its mass is the denominator of ``p_rows``.  With these, beta (mean_r mu[r] - mu) is the gradient of the
        mean marginal log-likelihood of incomplete data (``learn.fit_incomplete``).  A row of probability zero raises
        ValueError naming it.  A state the engine left deferred stays deferred.  A row fixes at most 28 qubits of a
        shard, the ancillas included (the engine refuses a row beyond that, naming it).  ``circuit``: a lowering of this
        circuit (``transpile``) to run in its place."""
        n, W = self._n, self._n + self._num_cliques + 1
        rows = np.asarray(rows)
        if rows.ndim != 2 or rows.shape[1] != n:
            raise ValueError("rows have shape %r, the model has %d variables" % (rows.shape, n))
        if rows.size and not np.isin(rows, (-1, 0, 1)).all():
            raise ValueError("a row entry is 0, 1 or -1 (unobserved)")
        run = self if circuit is None else circuit
        if self._with_measurements:
            backend.run(run, shots=0, post_select=self.post_selection(), **run_options)
        else:
            backend.run(run, shots=0, **run_options)
        anc = {q: 0 for q in range(n, W)}
        fixed_rows = []
        for row in rows:
            f = dict(anc)
            f.update({n - 1 - v: int(row[v]) for v in range(n) if row[v] >= 0})
            fixed_rows.append(f)
        fixed_rows.append(anc)
        groups = [[n - 1 - v for v in reversed(C)] for C in self._cliques]
        out, mass = backend.marginals_rows(groups, fixed_rows)
        norm = backend.last_engine.norm()
        if not mass[-1] > 0:
            raise ValueError("the post-selected outcome has zero probability")
        for r in range(rows.shape[0]):
            if not mass[r] > 0:
                raise ValueError("row %d has zero probability" % r)
        B = rows.shape[0]
        return out[:B] / mass[:B, None], mass[:B] / mass[-1], mass[-1] / norm

    def predict_proba(self, backend, rows, variable, circuit=None, **run_options):
        """P(x_variable = 1 | observed part of row r) for every row of ``rows`` (as in ``conditional_marginals``, which
        it calls once): read off the marginals of the first clique that contains the variable; a variable the row
        observes returns its value."""
        variable = int(variable)
        hit = [(ci, C) for ci, C in enumerate(self._cliques) if variable in C]
        if not hit:
            raise ValueError("variable %d is in no clique" % variable)
        ci, C = hit[0]
        mu = self.conditional_marginals(backend, rows, circuit=circuit, **run_options)[0]
        off = sum(2 ** len(D) for D in self._cliques[:ci])
        # y counts the clique states with the first variable of C most significant
        sel = [y for y in range(2 ** len(C)) if (y >> (len(C) - 1 - list(C).index(variable))) & 1]
        return mu[:, [off + y for y in sel]].sum(axis=1)

    def map_states(self, backend, k=1, evidence=None, circuit=None, **run_options):
        """The k most probable configurations of the Gibbs state this circuit prepares, given ``evidence`` ({variable:
        0/1}), from ONE run and one conditioned device pass -- exact MAP inference (k = 1) and its top-k form:
        ``(x, p, p_condition)`` with ``x`` an int array (m, n), x[i, v] the value of variable v, ``p`` their
        probabilities given the evidence, descending (equal p by ascending index, variable v on bit n-1-v; see
        ``QsvBackend.top_states`` for exact ties at the k-th place), and ``p_condition`` the probability that every
        ancilla and the AND scratch qubit read 0 AND the evidence holds.  Only the amplitudes that match are read, and
        a state the engine left deferred stays deferred.  m = min(k, matching states with p > 0).  ``circuit``: a
        lowering of this circuit (``transpile``) to run in its place."""
        n, W = self._n, self._n + self._num_cliques + 1
        k = int(k)
        if not 1 <= k <= mrf.MAP_MAX_K:
            raise ValueError("k = %d, 1..%d supported" % (k, mrf.MAP_MAX_K))
        fixed = {q: 0 for q in range(n, W)}
        for v, b in (evidence or {}).items():
            if not 0 <= int(v) < n:
                raise ValueError("evidence variable %d not in 0..%d" % (int(v), n - 1))
            fixed[n - 1 - int(v)] = int(bool(b))
        run = self if circuit is None else circuit
        if self._with_measurements:
            backend.run(run, shots=0, post_select=self.post_selection(), **run_options)
        else:
            backend.run(run, shots=0, **run_options)
        idx, p_raw = backend.top_states(k, fixed)
        # the mass of the same condition: one more pass over the sub-cube, the bits marginals() would divide by
        _, mass = backend.marginals([[]], fixed)
        norm = backend.last_engine.norm()
        if not mass > 0:
            raise ValueError("the post-selected outcome has zero probability")
        return mrf.states_of(idx & np.uint64((1 << n) - 1), n), p_raw / mass, mass / norm

    def post_selection(self):
        """``{classical bit: 0}`` for every clique ancilla: the branch in which the circuit prepares the Gibbs state
        (real part extraction succeeds when the ancilla reads 0, QCMRF.py:239).  For ``backend.run(self, shots,
        post_select=self.post_selection())``: every shot is then a Gibbs sample, and the metadata entry
        ``post_select_probability`` is the success probability."""
        if not self._with_measurements:
            raise ValueError("post_selection() needs the ancilla measurements: build the circuit with_measurements=True")
        return {self._n + 1 + i: 0 for i in range(self._num_cliques)}

    # ---- circuit construction (QCMRF.py:199-243) ---------------------------------------------
    def _clique_unitary(self, index, C, first_param):
        """cU_C: for every clique state y, AND . cp(2 gamma_y) . AND on (variables, scratch, ancilla)."""
        n = self._n
        sub = QuantumCircuit(n + 2, name='cU_C' + str(index))
        wires = [(n - 1) - v for v in C] + [n]
        for off, y in enumerate(itertools.product([0, 1], repeat=len(C))):
            g = self.gamma[first_param + off]
            if np.isclose(g, 0):
                continue
            flags = (np.array(y) * 2 - 1).tolist()
            # a fresh AND per append, compute and uncompute alike, exactly as QCMRF.py:225,227: the engine's
            # ingest recognises the blocks by content, however many distinct objects spell them
            sub.append(AND(len(C), flags), wires)
            sub.cp(2 * g, n, n + 1)
            sub.append(AND(len(C), flags), wires)
        return sub

    def _build(self):
        n = self._n
        for q in range(n):
            self.h(q)
        if self._with_barriers:
            self.barrier()

        if self._theta is None and self._gamma is None:
            # one scalar draw per parameter from the global numpy RNG, as QCMRF.py:210-213
            self._theta = [np.random.uniform(low=-5.0, high=0) for _ in range(self._dim)]

        main = list(range(n + 1))
        first = 0
        for ii, C in enumerate(self._cliques):
            anc = n + 1 + ii
            cu = self._clique_unitary(ii, C, first)
            first += 2 ** len(C)
            # real-part extraction: H cU X cU^dagger X H on the clique's ancilla
            self.h(anc)
            self.append(cu, main + [anc])
            self.x([anc])
            self.append(cu.inverse(), main + [anc])
            self.x([anc])
            self.h(anc)
            if self._with_measurements:
                self.measure(anc, anc)       # success <=> ancilla reads 0
            if self._with_barriers:
                self.barrier()
        if self._with_measurements:
            self.measure(range(n), range(n))


# ---- post-processing (QCMRF.py:247-284) ---------------------------------------------------------

def fidelity(P, Q):
    """Squared Bhattacharyya coefficient of two pmfs (entries that are <= 0 in either are skipped)."""
    P, Q = np.asarray(P, dtype=np.float64), np.asarray(Q, dtype=np.float64)
    both = (P > 0) & (Q > 0)
    return float(np.sum(np.sqrt(P[both] * Q[both]))) ** 2


def KL(P, Q):
    """Kullback-Leibler divergence sum P log(P/Q) over the common support."""
    P, Q = np.asarray(P, dtype=np.float64), np.asarray(Q, dtype=np.float64)
    both = (P > 0) & (Q > 0)
    return float(np.sum(P[both] * np.log(P[both] / Q[both])))


def extract_probs(R, n, a):
    """Counts dict -> (conditional pmf over the n variable bits given all ``a`` high bits are
    '0', success rate).  Key layout: ``'0'*a + x_0 x_1 ... x_{n-1}``."""
    P = np.zeros(2 ** n)
    head = '0' * a
    for i in range(2 ** n):
        key = head + format(i, '0{}b'.format(n)) if n > 0 else head
        if key in R:
            P[i] += R[key]
    z = np.sum(P)
    z0 = 0
    for key in R:
        z0 += R[key]
    if z == 0:
        return P, 0
    return P / z, z / z0
