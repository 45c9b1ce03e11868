"""Pauli noise models with the names and conventions of ``qiskit_aer.noise``.

    from qcmrf_amd.noise import NoiseModel, depolarizing_error, ReadoutError
    nm = NoiseModel()
    nm.add_all_qubit_quantum_error(depolarizing_error(1e-3, 1), ["sx", "x", "id"])
    nm.add_all_qubit_quantum_error(depolarizing_error(1e-2, 2), ["cx"])
    nm.add_all_qubit_readout_error(ReadoutError([[0.98, 0.02], [0.02, 0.98]]))
    counts = backend.run(circuits, shots=10000, noise_model=nm).result().get_counts()

Only Pauli channels (and readout errors) are represented: every ``QuantumError`` is a table of
4^n probabilities over the n-qubit Pauli group, run on the device as one random Pauli per shot
(a trajectory, ``qsv_noisy_sample``).

Pauli index order (shared with the encoder ``program.encode`` and the kernel ``qsv_noise.hip``):
index p of an n-qubit Pauli holds, for error qubit j, an x bit ``p >> 2j & 1`` and a z bit
``p >> 2j+1 & 1``; (x, z) = (0, 0) I, (1, 0) X, (0, 1) Z, (1, 1) Y.  The product of two Paulis is
the XOR of their indices, up to a phase.

Labels follow Qiskit: the RIGHTMOST character acts on error qubit 0, which is ``qargs[0]`` of the
gate the error is attached to ('XI' on ``cx(c, t)`` is X on t).  Errors act AFTER the gate.
"""
from __future__ import annotations

import numpy as np

_TOL = 1e-12
_XZ = {"I": (0, 0), "X": (1, 0), "Z": (0, 1), "Y": (1, 1)}
_CHAR = {v: k for k, v in _XZ.items()}
_NEVER = ("measure", "reset")


def label_to_index(label):
    """Qiskit Pauli label -> Pauli index (see the module docstring)"""
    n = len(label)
    p = 0
    for j in range(n):
        c = label[n - 1 - j].upper()
        if c not in _XZ:
            raise ValueError("%r is not a Pauli label (characters I, X, Y, Z)" % (label,))
        x, z = _XZ[c]
        p |= x << (2 * j) | z << (2 * j + 1)
    return p


def index_to_label(p, n):
    return "".join(_CHAR[((p >> (2 * j)) & 1, (p >> (2 * j + 1)) & 1)] for j in reversed(range(n)))


class QuantumError:
    """An n-qubit Pauli channel: ``probabilities[p]`` is the chance of Pauli index p."""

    def __init__(self, probabilities, num_qubits):
        n = int(num_qubits)
        if n < 1 or n > 2:
            raise ValueError("Pauli errors on %d qubits are not supported (1 or 2)" % n)
        p = np.array(probabilities, dtype=np.float64).ravel()
        if p.size != 4 ** n:
            raise ValueError("a %d-qubit Pauli error needs %d probabilities, got %d" % (n, 4 ** n, p.size))
        if not np.all(np.isfinite(p)) or (p < -_TOL).any():
            raise ValueError("Pauli error probabilities must be finite and non-negative")
        if abs(p.sum() - 1.0) > _TOL:
            raise ValueError("Pauli error probabilities sum to %.17g, not 1" % p.sum())
        p[p < 0] = 0.0
        p.setflags(write=False)
        self._p = p
        self._n = n

    @property
    def num_qubits(self):
        return self._n

    @property
    def probabilities(self):
        """4^n probabilities in Pauli index order (read-only array)"""
        return self._p

    def is_ideal(self):
        return bool(self._p[0] >= 1.0 - _TOL)

    def to_dict(self):
        """{Qiskit label: probability} for the Paulis with non-zero probability"""
        return {index_to_label(i, self._n): float(v) for i, v in enumerate(self._p) if v > 0}

    def compose(self, other):
        """``other`` after ``self``: the Pauli tables convolve over the Pauli group (phases dropped)"""
        other = _as_error(other)
        if other.num_qubits != self._n:
            raise ValueError("cannot compose a %d-qubit error with a %d-qubit one" % (self._n, other.num_qubits))
        idx = np.arange(4 ** self._n)
        out = np.zeros(4 ** self._n)
        for b, q in enumerate(other.probabilities):
            if q:
                out[idx ^ b] += self._p * q
        return QuantumError(out / out.sum(), self._n)

    def tensor(self, other):
        """``self`` (x) ``other``: ``other`` acts on error qubit 0, ``self`` on error qubit 1 (Qiskit order)"""
        other = _as_error(other)
        if self._n + other.num_qubits > 2:
            raise ValueError("tensor products beyond 2 qubits are not supported")
        p = np.outer(self._p, other.probabilities).ravel()          # index = self_index * 4 + other_index
        return QuantumError(p / p.sum(), 2)

    def expand(self, other):
        """``other`` (x) ``self``"""
        return _as_error(other).tensor(self)

    def __eq__(self, other):
        return isinstance(other, QuantumError) and other.num_qubits == self._n and np.allclose(other._p, self._p, atol=_TOL, rtol=0)

    __hash__ = None

    def __repr__(self):
        return "QuantumError(%s)" % self.to_dict()


def _as_error(e):
    if not isinstance(e, QuantumError):
        raise TypeError("expected a qcmrf_amd.noise.QuantumError, got %s" % type(e).__name__)
    return e


def pauli_error(noise_ops):
    """``pauli_error([('X', p), ('I', 1 - p)])``: a Pauli channel from (label, probability) pairs"""
    noise_ops = list(noise_ops)
    if not noise_ops:
        raise ValueError("pauli_error needs at least one (label, probability) pair")
    n = len(noise_ops[0][0])
    p = np.zeros(4 ** n) if 1 <= n <= 2 else None
    if p is None:
        raise ValueError("Pauli errors on %d qubits are not supported (1 or 2)" % n)
    for label, prob in noise_ops:
        if len(label) != n:
            raise ValueError("Pauli labels of different lengths: %r and %r" % (noise_ops[0][0], label))
        prob = float(prob)
        if not prob >= 0.0:
            raise ValueError("probability %r of %r is negative" % (prob, label))
        p[label_to_index(label)] += prob
    return QuantumError(p, n)


def depolarizing_error(param, num_qubits):
    """Aer's depolarizing error: P(I) = 1 - lam (4^n - 1) / 4^n, every other Pauli lam / 4^n,
    for 0 <= lam <= 4^n / (4^n - 1)"""
    n = int(num_qubits)
    if n not in (1, 2):
        raise ValueError("depolarizing errors on %d qubits are not supported (1 or 2)" % n)
    lam = float(param)
    d = 4 ** n
    if not 0.0 <= lam <= d / (d - 1.0):
        raise ValueError("depolarizing parameter %r outside [0, %g] for %d qubit(s)" % (param, d / (d - 1.0), n))
    p = np.full(d, lam / d)
    p[0] = 1.0 - lam * (d - 1) / d
    return QuantumError(p, n)


class ReadoutError:
    """One-qubit readout error ``[[P(0|0), P(1|0)], [P(0|1), P(1|1)]]``: rows are the ideal outcome,
    columns the recorded one"""

    def __init__(self, probabilities):
        m = np.array(probabilities, dtype=np.float64)
        if m.shape != (2, 2):
            raise ValueError("a readout error is a 2 x 2 matrix for one qubit, got shape %s" % (m.shape,))
        if not np.all(np.isfinite(m)) or (m < 0).any() or (m > 1).any():
            raise ValueError("readout probabilities must lie in [0, 1]")
        if np.abs(m.sum(axis=1) - 1.0).max() > _TOL:
            raise ValueError("each row of a readout error must sum to 1, got %s" % m.sum(axis=1).tolist())
        m.setflags(write=False)
        self._m = m

    @property
    def number_of_qubits(self):
        return 1

    @property
    def probabilities(self):
        return self._m

    def flips(self):
        """(P(flip | 0), P(flip | 1))"""
        return float(self._m[0, 1]), float(self._m[1, 0])

    def is_ideal(self):
        return self._m[0, 1] == 0 and self._m[1, 0] == 0

    def __repr__(self):
        return "ReadoutError(%s)" % self._m.tolist()


def _names(instructions):
    names = [instructions] if isinstance(instructions, str) else list(instructions)
    out = []
    for nm in names:
        nm = getattr(nm, "name", nm)
        if not isinstance(nm, str):
            raise TypeError("instruction names are strings, got %r" % (nm,))
        if nm in _NEVER:
            raise ValueError("errors on %r are not supported; use a ReadoutError for measurement noise" % nm)
        if nm == "barrier":
            raise ValueError("a barrier never takes an error")
        out.append(nm)
    return out


class NoiseModel:
    """Pauli gate errors and readout errors, keyed by instruction name as in ``qiskit_aer.noise.NoiseModel``.

    A local error (``add_quantum_error``) replaces the all-qubit error of the same instruction on exactly those
    qubits (in that order); adding a second error for the same key composes it after the first."""

    def __init__(self):
        self._default = {}            # name -> QuantumError
        self._local = {}              # (name, qubits) -> QuantumError
        self._ro_default = None
        self._ro_local = {}           # qubit -> ReadoutError

    def add_all_qubit_quantum_error(self, error, instructions):
        error = _as_error(error)
        for nm in _names(instructions):
            old = self._default.get(nm)
            self._default[nm] = error if old is None else old.compose(error)

    def add_quantum_error(self, error, instructions, qubits):
        error = _as_error(error)
        qs = tuple(int(q) for q in qubits)
        if len(qs) != error.num_qubits:
            raise ValueError("a %d-qubit error cannot act on qubits %s" % (error.num_qubits, list(qs)))
        if len(set(qs)) != len(qs) or min(qs) < 0:
            raise ValueError("invalid qubits %s" % (list(qs),))
        for nm in _names(instructions):
            old = self._local.get((nm, qs))
            self._local[(nm, qs)] = error if old is None else old.compose(error)

    def add_all_qubit_readout_error(self, error):
        if not isinstance(error, ReadoutError):
            raise TypeError("expected a qcmrf_amd.noise.ReadoutError, got %s" % type(error).__name__)
        self._ro_default = error

    def add_readout_error(self, error, qubits):
        if not isinstance(error, ReadoutError):
            raise TypeError("expected a qcmrf_amd.noise.ReadoutError, got %s" % type(error).__name__)
        qs = [int(q) for q in qubits]
        if len(qs) != 1:
            raise ValueError("a one-qubit readout error needs exactly one qubit, got %s" % qs)
        self._ro_local[qs[0]] = error

    # ---- queries (ingest) ------------------------------------------------------------------
    def is_ideal(self):
        """True if the model holds no error at all (an empty model runs the ideal path)"""
        return not (self._default or self._local or self._ro_default is not None or self._ro_local)

    @property
    def noise_instructions(self):
        return sorted(set(self._default) | {k[0] for k in self._local})

    def quantum_error(self, name, qubits):
        """the error that follows instruction ``name`` on ``qubits`` (a tuple), or None; an all-qubit error
        of another arity than the gate raises ValueError"""
        e = self._local.get((name, qubits))
        if e is not None:
            return e
        e = self._default.get(name)
        if e is not None and e.num_qubits != len(qubits):
            raise ValueError("a %d-qubit error is attached to %r, which acts on %d qubit(s)"
                             % (e.num_qubits, name, len(qubits)))
        return e

    def readout_flips(self, qubit):
        """(P(flip | 0), P(flip | 1)) of a measurement of ``qubit``, or None"""
        e = self._ro_local.get(int(qubit), self._ro_default)
        return None if e is None else e.flips()

    def __repr__(self):
        return "NoiseModel(%d all-qubit, %d local errors; readout: %s)" % (
            len(self._default), len(self._local),
            "all qubits" if self._ro_default is not None else ("%d qubits" % len(self._ro_local) if self._ro_local else "none"))
