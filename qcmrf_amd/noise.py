"""Noise models with the names and conventions of ``qiskit_aer.noise``: Pauli channels, one- and two-qubit Kraus channels.

    from qcmrf_amd.noise import NoiseModel, depolarizing_error, ReadoutError
    nm = NoiseModel()
    nm.add_all_qubit_quantum_error(depolarizing_error(1e-3, 1), ["sx", "x", "id"])
    nm.add_all_qubit_quantum_error(depolarizing_error(1e-2, 2), ["cx"])
    nm.add_all_qubit_readout_error(ReadoutError([[0.98, 0.02], [0.02, 0.98]]))
    counts = backend.run(circuits, shots=10000, noise_model=nm).result().get_counts()

A Pauli ``QuantumError`` is a table of 4^n probabilities over the n-qubit Pauli group, run on the device as one random
Pauli per shot (a trajectory, ``qsv_noisy_sample``).  One-qubit Kraus channels are represented too:

    from qcmrf_amd.noise import thermal_relaxation_error, amplitude_damping_error, kraus_error
    t = thermal_relaxation_error(100e3, 80e3, 35.0)                       # t1, t2, gate time in one unit
    nm.add_all_qubit_quantum_error(t, ["sx", "x", "id"])
    nm.add_all_qubit_quantum_error(t.expand(t).compose(depolarizing_error(1e-2, 2)), ["cx"])

``kraus_error``, ``amplitude_damping_error``, ``phase_damping_error``, ``phase_amplitude_damping_error``,
``thermal_relaxation_error`` and ``reset_error`` have Aer's names and argument order.  A one-qubit non-Pauli error holds
its 4 x 4 superoperator (column-stacking: S = sum_k conj(K_k) (x) K_k) and, unless Kraus operators were given, gets its
canonical Kraus set from the eigen-decomposition of its Choi matrix (at most four operators, descending eigenvalues).  A
two-qubit error is an ordered list of terms, each a Pauli table on both qubits or a one-qubit channel on error qubit j:
tensor products of one-qubit channels composed with two-qubit Pauli errors, which is how Aer's device models build
their ``cx`` errors.  On the device a channel term is one ``kraus`` op: per shot the kernel reduces the branch weights
<psi|K_k^dg K_k|psi> over the trajectory's state, draws one k, applies K_k and renormalises (``qsv_noise.hip``).

A general two-qubit channel is a third kind of term, one dense ``kraus2`` op of up to 16 operators of 4 x 4:

    from qcmrf_amd.noise import two_qubit_kraus_error, coherent_unitary_error, mixed_unitary_error
    zx = np.kron(X, Z)                                                    # Z on error qubit 0 (the control), X on error qubit 1
    over = coherent_unitary_error(scipy.linalg.expm(-0.5j * 0.05 * zx))   # over-rotation of the cross-resonance pulse
    nm.add_all_qubit_quantum_error(over.compose(depolarizing_error(1e-2, 2)), ["cx"])

``two_qubit_kraus_error`` takes the operators, ``coherent_unitary_error`` one unitary (2 x 2 or 4 x 4), ``mixed_unitary_error``
(unitary, probability) pairs.  Matrix index bit j is error qubit j (Aer's little-endian order: ``np.kron(A1, A0)`` has A0 on error
qubit 0).  Such an error holds its 16 x 16 superoperator; composing it with anything else on the two qubits gives one dense term,
the product of the superoperators, so a gate is followed by one record however its error was put together.

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


_PAULIS = (np.eye(2, dtype=np.complex128), np.array([[0, 1], [1, 0]], dtype=np.complex128),
           np.array([[1, 0], [0, -1]], dtype=np.complex128), np.array([[0, -1j], [1j, 0]], dtype=np.complex128))   # I X Z Y
_EIG_DROP = 1e-14


def _superop_of_kraus(ks):
    """sum_k conj(K_k) (x) K_k: acts on the column-stacked density matrix (rho_ij at index i + 2j)"""
    return sum(np.kron(k.conj(), k) for k in ks)


def _superop_of_pauli(p):
    return sum(w * np.kron(P.conj(), P) for w, P in zip(p, _PAULIS))


def _dim(S):
    """2 for a one-qubit superoperator (4 x 4), 4 for a two-qubit one (16 x 16)"""
    return 2 if S.shape[0] == 4 else 4


def _choi(S):
    """Choi matrix sum_k vec(K_k) vec(K_k)^dg (vec column-stacking) of a one- or two-qubit superoperator"""
    d = _dim(S)
    return S.reshape(d, d, d, d).transpose(3, 1, 2, 0).reshape(d * d, d * d)


def _canonical_kraus(S):
    """<= 4 (two qubits: <= 16) Kraus operators from the eigen-decomposition of the Choi matrix, descending eigenvalues;
    eigenvalues below 1e-14 are dropped; each operator's phase is fixed by making its largest entry real and positive"""
    d = _dim(S)
    lam, vec = np.linalg.eigh(_choi(S))
    out = []
    for i in np.argsort(-lam, kind="stable"):
        if lam[i] < _EIG_DROP:
            continue
        k = np.sqrt(lam[i]) * vec[:, i].reshape(d, d).T
        big = k.ravel()[np.argmax(np.abs(k.ravel()))]
        out.append(k * (abs(big) / big))
    return out


def _check_cptp(S, what):
    lam = np.linalg.eigvalsh(_choi(S))
    if not np.all(np.isfinite(S)) or lam.min() < -1e-10:
        raise ValueError("%s is not completely positive (Choi eigenvalue %.3g)" % (what, lam.min()))
    tp = S[0] + S[3]                                           # trace of the output as a functional of the input
    if np.abs(tp - np.array([1, 0, 0, 1])).max() > 1e-10:
        raise ValueError("%s does not preserve the trace" % what)


def _paulis2():
    """the 16 two-qubit Paulis in Pauli index order: index p has error qubit 0 in its low two bits"""
    return [np.kron(_PAULIS[p >> 2], _PAULIS[p & 3]) for p in range(16)]


def _superop_of_pauli2(p):
    return sum(w * np.kron(P.conj(), P) for w, P in zip(p, _paulis2()) if w)


def _pauli_table_of(S):
    """the 4 (two qubits: 16) probabilities if the superoperator is a Pauli channel, else None"""
    C = _choi(S)
    two = _dim(S) == 4
    group = _paulis2() if two else _PAULIS
    p = np.array([np.real(np.vdot(P.T.ravel(), C @ P.T.ravel())) / float(len(group)) for P in group])
    if np.abs(S - (_superop_of_pauli2(p) if two else _superop_of_pauli(p))).max() > _TOL or (p < -_TOL).any():
        return None
    p = np.clip(p, 0.0, None)
    return p / p.sum()


class _Chan:
    """a one-qubit channel (a "chan" term) or a dense two-qubit one (a "k2" term): its superoperator and, when they were
    given, its Kraus operators"""
    __slots__ = ("S", "given")

    def __init__(self, S, given=None):
        self.S = S
        self.given = given

    def kraus(self):
        return list(self.given) if self.given is not None else _canonical_kraus(self.S)


def _superop_of_term(kind, qs, x):
    """the 16 x 16 superoperator of one term of a two-qubit error"""
    if kind == "k2":
        return x.S
    if kind == "pauli":
        return _superop_of_pauli2(x)
    I2 = _PAULIS[0]
    return sum(np.kron(k.conj(), k) for k in (np.kron(I2, k) if qs[0] == 0 else np.kron(k, I2) for k in x.kraus()))


def _merge(terms):
    """ordered terms with adjacent terms of one shape on the same qubits merged (one-qubit channels on different qubits
    commute, so a channel also merges with the last channel on its qubit across channels on the other one).  A dense
    two-qubit term takes everything else with it: the terms become one "k2" term, the product of their superoperators --
    one record behind the gate instead of several; a single term keeps the operators it was given"""
    terms = list(terms)
    if len(terms) > 1 and any(kind == "k2" for kind, _, _ in terms):
        S = np.eye(16, dtype=np.complex128)
        for kind, qs, x in terms:
            S = _superop_of_term(kind, qs, x) @ S
        return [("k2", (0, 1), _Chan(S))]
    out = []
    for kind, qs, x in terms:
        if kind == "pauli":
            if out and out[-1][0] == "pauli":
                out[-1] = ("pauli", qs, _convolve(out[-1][2], x))
            else:
                out.append((kind, qs, x))
            continue
        k = len(out) - 1
        while k >= 0 and out[k][0] == "chan" and out[k][1] != qs:
            k -= 1
        if k >= 0 and out[k][0] == "chan":
            out[k] = ("chan", qs, _Chan(x.S @ out[k][2].S))
        else:
            out.append((kind, qs, x))
    return out


def _convolve(p, q):
    """Pauli table q after Pauli table p: the convolution over the Pauli group (phases dropped)"""
    idx = np.arange(p.size)
    out = np.zeros(p.size)
    for b, w in enumerate(q):
        if w:
            out[idx ^ b] += p * w
    return out / out.sum()


class QuantumError:
    """An n-qubit error (n = 1 or 2).  ``QuantumError(probabilities, n)`` is a Pauli channel: ``probabilities[p]`` is the
    chance of Pauli index p.  The constructors below and ``compose`` / ``tensor`` also give one-qubit Kraus channels,
    two-qubit products of them and dense two-qubit channels (module docstring)."""

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
        self._chain = None            # non-Pauli errors: ordered ("pauli", (0, 1), table) / ("chan", (j,), _Chan) terms,
                                      # or one ("k2", (0, 1), _Chan) term: a dense two-qubit channel
        self._emit = None

    @classmethod
    def _from_terms(cls, terms, n):
        """an error from ordered terms; one that is a single Pauli table becomes a plain Pauli error"""
        terms = _merge(terms)
        if len(terms) == 1 and terms[0][0] == "pauli":
            return cls(terms[0][2], n)
        e = cls.__new__(cls)
        e._p, e._n, e._chain, e._emit = None, n, terms, None
        return e

    def _terms(self):
        return [("pauli", tuple(range(self._n)), self._p)] if self._chain is None else list(self._chain)

    def _chan(self):
        """this one-qubit error as a _Chan (Pauli tables are lifted)"""
        if self._n != 1:
            raise ValueError("a two-qubit error has no one-qubit superoperator")
        return _Chan(_superop_of_pauli(self._p)) if self._chain is None else self._chain[0][2]

    @property
    def num_qubits(self):
        return self._n

    def is_pauli(self):
        return self._chain is None

    @property
    def probabilities(self):
        """4^n probabilities in Pauli index order (read-only array); Pauli errors only"""
        if self._p is None:
            raise ValueError("this error is not a Pauli channel: it has terms() and, on one qubit, kraus()")
        return self._p

    def is_ideal(self):
        if self._chain is None:
            return bool(self._p[0] >= 1.0 - _TOL)
        return all(np.abs(x.S - np.eye(x.S.shape[0])).max() <= _TOL if k in ("chan", "k2") else x[0] >= 1.0 - _TOL
                   for k, _, x in self._chain)

    def to_dict(self):
        """{Qiskit label: probability} for the Paulis with non-zero probability"""
        return {index_to_label(i, self._n): float(v) for i, v in enumerate(self.probabilities) if v > 0}

    def kraus(self):
        """the Kraus operators of a one-qubit error: as given to ``kraus_error``, else canonical (Pauli errors:
        sqrt(p) P for every Pauli with p > 0)"""
        if self._n != 1:
            raise ValueError("kraus() is for one-qubit errors; a two-qubit error has terms()")
        if self._chain is None:
            return [np.sqrt(w) * P for w, P in zip(self._p, _PAULIS) if w > 0]
        return [k.copy() for k in self._chain[0][2].kraus()]

    def superoperator(self):
        """the 4 x 4 superoperator of a one-qubit error on the column-stacked density matrix (rho_ij at index i + 2j);
        for a two-qubit error the 16 x 16 one, error qubit 0 the low bit of the row and column indices"""
        if self._n == 1:
            return self._chan().S.copy()
        S = np.eye(16, dtype=np.complex128)
        for kind, qs, x in self._terms():
            S = _superop_of_term(kind, qs, x) @ S
        return S

    def terms(self):
        """what ingest walks, in order: ("pauli", error qubits, probability table), ("kraus", (error qubit,), stack of m
        2 x 2 operators) or ("kraus2", (0, 1), stack of m 4 x 4 operators, index bit j on error qubit j).  A channel without
        given Kraus operators that is a Pauli channel comes as "pauli"."""
        if self._emit is None:
            out = []
            for kind, qs, x in self._terms():
                if kind in ("chan", "k2"):
                    d = _dim(x.S)
                    p = _pauli_table_of(x.S) if x.given is None else None
                    if p is not None:
                        p.setflags(write=False)
                        out.append(("pauli", qs, p))
                    else:
                        ks = np.array(x.kraus(), dtype=np.complex128).reshape(-1, d, d)
                        ks.setflags(write=False)
                        out.append(("kraus" if kind == "chan" else "kraus2", qs, ks))
                else:
                    out.append((kind, qs, x))
            self._emit = tuple(out)
        return self._emit

    def compose(self, other):
        """``other`` after ``self``.  Pauli tables convolve over the Pauli group (phases dropped); one-qubit channels
        multiply their superoperators (a Pauli table is lifted when it meets a non-Pauli partner); on two qubits the
        ordered terms are concatenated and adjacent terms of one shape on the same qubits merged; with a dense two-qubit
        term among them they all become one dense term, the product of the superoperators"""
        other = _as_error(other)
        if other.num_qubits != self._n:
            raise ValueError("cannot compose a %d-qubit error with a %d-qubit one" % (self._n, other.num_qubits))
        if self._chain is None and other._chain is None:
            idx = np.arange(4 ** self._n)
            out = np.zeros(4 ** self._n)
            for b, q in enumerate(other.probabilities):
                if q:
                    out[idx ^ b] += self._p * q
            return QuantumError(out / out.sum(), self._n)
        if self._n == 1:
            return QuantumError._from_terms([("chan", (0,), _Chan(other._chan().S @ self._chan().S))], 1)
        return QuantumError._from_terms(self._terms() + other._terms(), 2)

    def tensor(self, other):
        """``self`` (x) ``other``: ``other`` acts on error qubit 0, ``self`` on error qubit 1 (Qiskit order)"""
        other = _as_error(other)
        if self._n + other.num_qubits > 2:
            raise ValueError("tensor products beyond 2 qubits are not supported")
        if self._chain is None and other._chain is None:
            p = np.outer(self._p, other.probabilities).ravel()          # index = self_index * 4 + other_index
            return QuantumError(p / p.sum(), 2)
        return QuantumError._from_terms([("chan", (0,), other._chan()), ("chan", (1,), self._chan())], 2)

    def expand(self, other):
        """``other`` (x) ``self``"""
        return _as_error(other).tensor(self)

    def __eq__(self, other):
        if not isinstance(other, QuantumError) or other.num_qubits != self._n:
            return False
        if self._chain is None and other._chain is None:
            return bool(np.allclose(other._p, self._p, atol=_TOL, rtol=0))
        return bool(np.allclose(other.superoperator(), self.superoperator(), atol=1e-10, rtol=0))

    __hash__ = None

    def __repr__(self):
        if self._chain is None:
            return "QuantumError(%s)" % self.to_dict()
        return "QuantumError(%d qubit(s): %s)" % (self._n, ", ".join(
            "%s on %s" % ("Pauli table" if k == "pauli" else "%d Kraus operators" % len(x.kraus()), list(qs))
            for k, qs, x in self._chain))


def _as_error(e):
    if not isinstance(e, QuantumError):
        raise TypeError("expected a qcmrf_amd.noise.QuantumError, got %s" % type(e).__name__)
    return e


def kraus_error(noise_ops):
    """a one-qubit channel from 1 to 4 Kraus operators (2 x 2), kept as given and in order; more than four are reduced
    to the canonical set.  sum K^dg K must be the identity to 1e-12.  4 x 4 operators are refused here: a general
    two-qubit Kraus set goes to ``two_qubit_kraus_error``"""
    ks = [np.array(k, dtype=np.complex128) for k in noise_ops]
    if not ks:
        raise ValueError("kraus_error needs at least one operator")
    if any(k.shape == (4, 4) for k in ks):
        raise ValueError("kraus_error takes 2 x 2 operators: a general two-qubit Kraus set (4 x 4 operators) goes to "
                         "two_qubit_kraus_error")
    if any(k.shape != (2, 2) for k in ks):
        raise ValueError("Kraus operators are 2 x 2 matrices, got shapes %s" % sorted({k.shape for k in ks}))
    if not all(np.all(np.isfinite(k)) for k in ks):
        raise ValueError("Kraus operators must be finite")
    tp = sum(k.conj().T @ k for k in ks)
    if np.abs(tp - np.eye(2)).max() > _TOL:
        raise ValueError("not a channel: sum K^dg K differs from the identity by %.3g" % np.abs(tp - np.eye(2)).max())
    S = _superop_of_kraus(ks)
    for k in ks:
        k.setflags(write=False)
    return QuantumError._from_terms([("chan", (0,), _Chan(S, ks if len(ks) <= 4 else None))], 1)


def two_qubit_kraus_error(noise_ops):
    """a two-qubit channel from 1 or more Kraus operators (4 x 4), matrix index bit j on error qubit j -- the gate's j-th
    qubit argument, Aer's little-endian order and the order of the two-qubit Pauli index.  Up to 16 operators are kept as
    given and in order; more are reduced to the canonical set (Choi eigenvalues below 1e-14 dropped, at most 16,
    descending).  sum K^dg K must be the identity to 1e-12."""
    ks = [np.array(k, dtype=np.complex128) for k in noise_ops]
    if not ks:
        raise ValueError("two_qubit_kraus_error needs at least one operator")
    if any(k.shape != (4, 4) for k in ks):
        raise ValueError("two-qubit Kraus operators are 4 x 4 matrices, got shapes %s" % sorted({k.shape for k in ks}))
    if not all(np.all(np.isfinite(k)) for k in ks):
        raise ValueError("Kraus operators must be finite")
    tp = sum(k.conj().T @ k for k in ks)
    if np.abs(tp - np.eye(4)).max() > _TOL:
        raise ValueError("not a channel: sum K^dg K differs from the identity by %.3g" % np.abs(tp - np.eye(4)).max())
    S = _superop_of_kraus(ks)
    for k in ks:
        k.setflags(write=False)
    return QuantumError._from_terms([("k2", (0, 1), _Chan(S, ks if len(ks) <= 16 else None))], 2)


def _unitary(u, what):
    u = np.array(u, dtype=np.complex128)
    if u.shape not in ((2, 2), (4, 4)):
        raise ValueError("%s is a 2 x 2 or 4 x 4 matrix, got shape %s" % (what, u.shape))
    if not np.all(np.isfinite(u)) or np.abs(u.conj().T @ u - np.eye(len(u))).max() > _TOL:
        raise ValueError("%s is not unitary to 1e-12" % what)
    return u


def coherent_unitary_error(unitary):
    """the unitary error rho -> U rho U^dg on one (2 x 2) or two (4 x 4) qubits: a Kraus set of one operator"""
    u = _unitary(unitary, "a coherent error")
    return kraus_error([u]) if len(u) == 2 else two_qubit_kraus_error([u])


def _pauli_index_of(u):
    """the Pauli index of a unitary that is a Pauli up to a phase, else None"""
    d = len(u)
    for p, P in enumerate(_PAULIS if d == 2 else _paulis2()):
        t = np.vdot(P, u) / d                              # tr(P^dg U) / d: modulus 1 only for a phase times P
        if abs(abs(t) - 1.0) <= _TOL:
            return p
    return None


def mixed_unitary_error(noise_ops):
    """``mixed_unitary_error([(U_0, p_0), (U_1, p_1), ...])``: U_k with probability p_k, on one or two qubits.  The
    probabilities are non-negative and sum to 1 to 1e-12; terms of probability 0 are dropped; K_k = sqrt(p_k) U_k, kept in
    order up to 4 operators on one qubit and 16 on two, canonical beyond that.  Unitaries that are all Paulis (up to a
    phase) make a Pauli error."""
    pairs = [(_unitary(u, "a term of a mixed-unitary error"), float(p)) for u, p in noise_ops]
    if not pairs:
        raise ValueError("mixed_unitary_error needs at least one (unitary, probability) pair")
    d = len(pairs[0][0])
    if any(len(u) != d for u, _ in pairs):
        raise ValueError("the unitaries of a mixed-unitary error differ in size")
    ps = np.array([p for _, p in pairs])
    if not np.all(np.isfinite(ps)) or (ps < 0).any():
        raise ValueError("mixed-unitary probabilities must be finite and non-negative")
    if abs(ps.sum() - 1.0) > _TOL:
        raise ValueError("mixed-unitary probabilities sum to %.17g, not 1" % ps.sum())
    pairs = [(u, p) for u, p in pairs if p > 0]
    idx = [_pauli_index_of(u) for u, _ in pairs]
    if all(i is not None for i in idx):
        table = np.zeros(d * d)
        for i, (_, p) in zip(idx, pairs):
            table[i] += p
        return QuantumError(table / table.sum(), 1 if d == 2 else 2)
    ks = [np.sqrt(p) * u for u, p in pairs]
    tp = sum(k.conj().T @ k for k in ks)                   # the identity up to the rounding of sum p: take it out
    ks = [k / np.sqrt(np.real(np.trace(tp)) / d) for k in ks]
    return kraus_error(ks) if d == 2 else two_qubit_kraus_error(ks)


def phase_amplitude_damping_error(param_amp, param_phase, excited_state_population=0):
    """Aer's combined damping channel: with a = param_amp, b = param_phase, p1 = the excited state population and
    c = 1 - a - b >= 0 the Kraus operators sqrt(1 - p1) {diag(1, sqrt c), sqrt a |0><1|, sqrt b diag(0, 1)} and
    sqrt(p1) {diag(sqrt c, 1), sqrt a |1><0|, sqrt b diag(1, 0)}"""
    a, b, p1 = float(param_amp), float(param_phase), float(excited_state_population)
    if not (0.0 <= a <= 1.0 and 0.0 <= b <= 1.0):
        raise ValueError("damping parameters %r, %r outside [0, 1]" % (param_amp, param_phase))
    if a + b > 1.0 + _TOL:
        raise ValueError("param_amp + param_phase = %.17g exceeds 1" % (a + b))
    if not 0.0 <= p1 <= 1.0:
        raise ValueError("excited state population %r outside [0, 1]" % (excited_state_population,))
    c = np.sqrt(max(0.0, 1.0 - a - b))
    sa, sb, s0, s1 = np.sqrt(a), np.sqrt(b), np.sqrt(1.0 - p1), np.sqrt(p1)
    ks = [s0 * np.diag([1.0, c]), s0 * sa * np.array([[0, 1], [0, 0]]), s0 * sb * np.diag([0.0, 1.0]),
          s1 * np.diag([c, 1.0]), s1 * sa * np.array([[0, 0], [1, 0]]), s1 * sb * np.diag([1.0, 0.0])]
    return kraus_error([k for k in ks if np.abs(k).max() > 0])


def amplitude_damping_error(param_amp, excited_state_population=0):
    return phase_amplitude_damping_error(param_amp, 0.0, excited_state_population)


def phase_damping_error(param_phase):
    return phase_amplitude_damping_error(0.0, param_phase, 0)


def _from_superop(S, what):
    S = np.asarray(S, dtype=np.complex128)
    _check_cptp(S, what)
    return QuantumError._from_terms([("chan", (0,), _Chan(S))], 1)


def thermal_relaxation_error(t1, t2, time, excited_state_population=0):
    """T1 / T2 relaxation over ``time`` (all three in one unit): with p_r = 1 - exp(-time / t1), e2 = exp(-time / t2),
    p1 = the excited state population and p0 = 1 - p1,
        rho00' = (1 - p1 p_r) rho00 + p0 p_r rho11,  rho11' = p1 p_r rho00 + (1 - p0 p_r) rho11,  rho01' = e2 rho01:
    one CPTP map for t2 <= t1 and for t1 < t2 <= 2 t1.  Trajectories agree with Aer's in distribution."""
    t1, t2, time, p1 = float(t1), float(t2), float(time), float(excited_state_population)
    if not (t1 > 0 and t2 > 0):
        raise ValueError("t1 and t2 must be positive (inf allowed), got %r, %r" % (t1, t2))
    if not (time >= 0 and np.isfinite(time)):
        raise ValueError("the gate time must be finite and >= 0, got %r" % (time,))
    if t2 > 2.0 * t1:
        raise ValueError("t2 = %r exceeds 2 t1 = %r" % (t2, 2.0 * t1))
    if not 0.0 <= p1 <= 1.0:
        raise ValueError("excited state population %r outside [0, 1]" % (excited_state_population,))
    pr, e2, p0 = -np.expm1(-time / t1), np.exp(-time / t2), 1.0 - p1
    S = np.array([[1.0 - p1 * pr, 0, 0, p0 * pr], [0, e2, 0, 0], [0, 0, e2, 0], [p1 * pr, 0, 0, 1.0 - p0 * pr]])
    return _from_superop(S, "thermal relaxation")


def reset_error(prob0, prob1=0):
    """with probability prob0 the qubit is set to |0>, with prob1 to |1>, otherwise it is left alone"""
    a, b = float(prob0), float(prob1)
    if not (a >= 0 and b >= 0 and a + b <= 1.0 + _TOL):
        raise ValueError("reset probabilities %r, %r must be non-negative and sum to at most 1" % (prob0, prob1))
    r0 = np.array([[1, 0, 0, 1], [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]], dtype=np.float64)
    r1 = r0[::-1].copy()
    return _from_superop(max(0.0, 1.0 - a - b) * np.eye(4) + a * r0 + b * r1, "reset error")


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
    """Gate errors (Pauli and Kraus) and readout errors, keyed by instruction name as in ``qiskit_aer.noise.NoiseModel``.

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
