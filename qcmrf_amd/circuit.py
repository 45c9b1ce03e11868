"""A small, Qiskit-free circuit container with Qiskit's *data model*.

The reference builds its circuits with ``qiskit.QuantumCircuit`` and ``qiskit.circuit.library.AND``
(/root/reference/QCMRF.py:7,9,13).  Qiskit is not installed in this image, so ``QCMRF(...)`` needs
something to derive from.  This module provides exactly the surface QCMRF.py touches -- ``h``,
``x``, ``cp``, ``measure``, ``barrier``, ``append``, ``inverse``, nested instructions with a
``definition`` -- using the attribute names the engine's duck-typed ingest reads on real Qiskit
objects too (``circuit.data[i].operation.name/.params/.definition``, ``.qubits``, ``.clbits``,
``circuit.find_bit(bit).index``, ``circuit.global_phase``).  When Qiskit *is* importable,
``qcmrf_amd.qcmrf`` derives from the real class instead and this file is not used.

It is a container, not a simulator: no matrices, no state.
"""
from __future__ import annotations

from collections import namedtuple

BitLocations = namedtuple("BitLocations", ("index", "registers"))

# name -> (num_qubits, num_params, inverse name or None for "negate params")
_STANDARD = {
    "h": (1, 0, "h"), "x": (1, 0, "x"), "y": (1, 0, "y"), "z": (1, 0, "z"), "id": (1, 0, "id"),
    "s": (1, 0, "sdg"), "sdg": (1, 0, "s"), "t": (1, 0, "tdg"), "tdg": (1, 0, "t"),
    "sx": (1, 0, "sxdg"), "sxdg": (1, 0, "sx"),
    "rx": (1, 1, None), "ry": (1, 1, None), "rz": (1, 1, None), "p": (1, 1, None),
    "cx": (2, 0, "cx"), "cz": (2, 0, "cz"), "swap": (2, 0, "swap"), "cp": (2, 1, None),
    "crz": (2, 1, None), "ccx": (3, 0, "ccx"),
}


class Bit:
    __slots__ = ("_register", "_index")

    def __init__(self, register=None, index=None):
        self._register, self._index = register, index

    def __repr__(self):
        return "%s(%s)" % (type(self).__name__, self._index)


class Qubit(Bit):
    pass


class Clbit(Bit):
    pass


class Register:
    def __init__(self, size, name, bit_type):
        self.name, self.size = name, size
        self._bits = [bit_type(self, i) for i in range(size)]

    def __len__(self):
        return self.size

    def __iter__(self):
        return iter(self._bits)

    def __getitem__(self, i):
        return self._bits[i]


class Instruction:
    """Counterpart of qiskit.circuit.Instruction (name, params, definition, condition)."""

    def __init__(self, name, num_qubits, num_clbits=0, params=(), definition=None):
        self.name = name
        self.num_qubits = num_qubits
        self.num_clbits = num_clbits
        self.params = list(params)
        self.definition = definition
        self.condition = None

    def c_if(self, classical, val):
        """condition the instruction on ``classical`` (a Clbit or a classical register) reading the integer ``val``, as
        qiskit.circuit.Instruction.c_if did before Qiskit 2.0: sets ``condition`` and returns the instruction"""
        if not isinstance(classical, (Clbit, Register)):
            raise TypeError("c_if takes a Clbit or a classical register, not %s" % type(classical).__name__)
        if int(val) < 0:
            raise ValueError("c_if compares with a non-negative integer, not %r" % (val,))
        self.condition = (classical, int(val))
        return self

    def inverse(self):
        if self.definition is not None:
            name = self.name[:-3] if self.name.endswith("_dg") else self.name + "_dg"
            inv = self.definition.inverse()
            inv.name = name
            return Instruction(name, self.num_qubits, self.num_clbits, self.params, inv)
        if self.name.startswith("mcx"):
            return Instruction(self.name, self.num_qubits)
        if self.name in _STANDARD:
            nq, npar, inv = _STANDARD[self.name]
            if inv is None:
                return Instruction(self.name, nq, 0, [-p for p in self.params])
            if self.name == "u":
                th, ph, lam = self.params
                return Instruction("u", 1, 0, [-th, -lam, -ph])
            return Instruction(inv, nq)
        if self.name == "u":
            th, ph, lam = self.params
            return Instruction("u", 1, 0, [-th, -lam, -ph])
        raise ValueError("cannot invert instruction %r" % self.name)

    def copy(self):
        return Instruction(self.name, self.num_qubits, self.num_clbits, list(self.params), self.definition)

    def __repr__(self):
        return "Instruction(name=%r, num_qubits=%d, params=%r)" % (self.name, self.num_qubits, self.params)


class InstructionSet:
    """what a gate method returns: the instructions it just added, so that ``qc.x(0).c_if(c, 1)`` reaches them
    (counterpart of qiskit.circuit.InstructionSet)"""

    def __init__(self, instructions):
        self.instructions = list(instructions)

    def c_if(self, classical, val):
        for ci in self.instructions:
            ci.operation.c_if(classical, val)
        return self

    def __len__(self):
        return len(self.instructions)

    def __getitem__(self, i):
        return self.instructions[i]


class IfElseOp(Instruction):
    """``if_else`` on all qubits and clbits of the circuit it was opened in: ``condition`` = (Clbit or register, value),
    ``blocks`` = (true body, else body or None), each a circuit over the same bits in the same order (counterpart of
    qiskit.circuit.IfElseOp)"""

    def __init__(self, condition, true_body, false_body=None):
        super().__init__("if_else", true_body.num_qubits, true_body.num_clbits)
        self.condition = condition
        self.blocks = (true_body, false_body)


class _ElseContext:
    def __init__(self, circuit, op):
        self._circuit, self._op = circuit, op

    def __enter__(self):
        if self._op.blocks[1] is not None:
            raise ValueError("this if_test has an else body already")
        self._circuit._open_body()
        return None

    def __exit__(self, exc_type, exc, tb):
        body = self._circuit._close_body()
        if exc_type is None:
            self._op.blocks = (self._op.blocks[0], body)
        return False


class _IfContext:
    """``with qc.if_test((c, 1)) as else_:`` -- the gates added inside go to the true body; ``with else_:`` opens the else body"""

    def __init__(self, circuit, condition):
        self._circuit, self._condition = circuit, condition

    def __enter__(self):
        self._circuit._open_body()
        self._else = _ElseContext(self._circuit, None)
        return self._else

    def __exit__(self, exc_type, exc, tb):
        body = self._circuit._close_body()
        if exc_type is None:
            op = IfElseOp(self._condition, body)
            self._else._op = op
            self._circuit._add(op, list(self._circuit.qubits), list(self._circuit.clbits))
        return False


class CircuitInstruction:
    """(operation, qubits, clbits) triple; also unpacks like the legacy tuple form."""
    __slots__ = ("operation", "qubits", "clbits")

    def __init__(self, operation, qubits=(), clbits=()):
        self.operation, self.qubits, self.clbits = operation, tuple(qubits), tuple(clbits)

    def __iter__(self):
        return iter((self.operation, list(self.qubits), list(self.clbits)))

    def __repr__(self):
        return "CircuitInstruction(%r, qubits=%r, clbits=%r)" % (self.operation, self.qubits, self.clbits)


class QuantumCircuit:
    """Counterpart of qiskit.QuantumCircuit for the calls QCMRF.py makes (QCMRF.py:78,205-243)."""

    def __init__(self, num_qubits=0, num_clbits=0, name=None, global_phase=0.0):
        self.name = name if name is not None else "circuit"
        self.global_phase = global_phase
        self._qreg = Register(int(num_qubits), "q", Qubit)
        self._creg = Register(int(num_clbits), "c", Clbit)
        self.qregs = [self._qreg] if num_qubits else []
        self.cregs = [self._creg] if num_clbits else []
        self.qubits = list(self._qreg)
        self.clbits = list(self._creg)
        self._qindex = {id(b): i for i, b in enumerate(self.qubits)}
        self._cindex = {id(b): i for i, b in enumerate(self.clbits)}
        self.data = []
        self._bodies = []                # open if_test bodies, innermost last: gates added meanwhile go there

    # ---- structure queries ---------------------------------------------------------
    @property
    def num_qubits(self):
        return len(self.qubits)

    @property
    def num_clbits(self):
        return len(self.clbits)

    def find_bit(self, bit):
        if id(bit) in self._qindex:
            return BitLocations(self._qindex[id(bit)], [(self._qreg, self._qindex[id(bit)])])
        if id(bit) in self._cindex:
            return BitLocations(self._cindex[id(bit)], [(self._creg, self._cindex[id(bit)])])
        raise ValueError("bit %r is not in this circuit" % (bit,))

    def size(self):
        return sum(1 for ci in self.data if ci.operation.name != "barrier")

    def count_ops(self):
        out = {}
        for ci in self.data:
            out[ci.operation.name] = out.get(ci.operation.name, 0) + 1
        return out

    def __len__(self):
        return len(self.data)

    # ---- argument plumbing ---------------------------------------------------------
    def _q(self, spec):
        """int | Qubit | iterable thereof -> list of Qubit"""
        if isinstance(spec, Qubit):
            return [spec]
        if isinstance(spec, (int,)) or hasattr(spec, "__index__"):
            return [self.qubits[int(spec)]]
        return [q for s in spec for q in self._q(s)]

    def _c(self, spec):
        if isinstance(spec, Clbit):
            return [spec]
        if isinstance(spec, (int,)) or hasattr(spec, "__index__"):
            return [self.clbits[int(spec)]]
        return [c for s in spec for c in self._c(s)]

    def _add(self, op, qubits, clbits=()):
        if len(set(id(q) for q in qubits)) != len(qubits):
            raise ValueError("duplicate qubit arguments in %s" % op.name)
        ci = CircuitInstruction(op, qubits, clbits)
        (self._bodies[-1].data if self._bodies else self.data).append(ci)
        return ci

    def _open_body(self):
        body = QuantumCircuit.__new__(QuantumCircuit)          # the same bit objects in the same order: a view, not a copy
        body.name, body.global_phase = "if_body", 0.0
        body._qreg, body._creg, body.qregs, body.cregs = self._qreg, self._creg, self.qregs, self.cregs
        body.qubits, body.clbits, body._qindex, body._cindex = self.qubits, self.clbits, self._qindex, self._cindex
        body.data, body._bodies = [], []
        self._bodies.append(body)

    def _close_body(self):
        return self._bodies.pop()

    def _broadcast_1q(self, name, qubit, params=()):
        return InstructionSet([self._add(Instruction(name, 1, 0, params), [q]) for q in self._q(qubit)])

    # ---- gates -----------------------------------------------------------------------
    def h(self, qubit): return self._broadcast_1q("h", qubit)
    def x(self, qubit): return self._broadcast_1q("x", qubit)
    def y(self, qubit): return self._broadcast_1q("y", qubit)
    def z(self, qubit): return self._broadcast_1q("z", qubit)
    def s(self, qubit): return self._broadcast_1q("s", qubit)
    def sdg(self, qubit): return self._broadcast_1q("sdg", qubit)
    def t(self, qubit): return self._broadcast_1q("t", qubit)
    def tdg(self, qubit): return self._broadcast_1q("tdg", qubit)
    def sx(self, qubit): return self._broadcast_1q("sx", qubit)
    def sxdg(self, qubit): return self._broadcast_1q("sxdg", qubit)
    def id(self, qubit): return self._broadcast_1q("id", qubit)
    def rx(self, theta, qubit): return self._broadcast_1q("rx", qubit, [theta])
    def ry(self, theta, qubit): return self._broadcast_1q("ry", qubit, [theta])
    def rz(self, phi, qubit): return self._broadcast_1q("rz", qubit, [phi])
    def p(self, lam, qubit): return self._broadcast_1q("p", qubit, [lam])
    def u(self, theta, phi, lam, qubit): return self._broadcast_1q("u", qubit, [theta, phi, lam])

    def cx(self, control, target):
        return InstructionSet([self._add(Instruction("cx", 2), self._q(control) + self._q(target))])

    def cz(self, control, target):
        return InstructionSet([self._add(Instruction("cz", 2), self._q(control) + self._q(target))])

    def swap(self, a, b):
        return InstructionSet([self._add(Instruction("swap", 2), self._q(a) + self._q(b))])

    def cp(self, theta, control, target):
        return InstructionSet([self._add(Instruction("cp", 2, 0, [theta]), self._q(control) + self._q(target))])

    def crz(self, theta, control, target):
        return InstructionSet([self._add(Instruction("crz", 2, 0, [theta]), self._q(control) + self._q(target))])

    def ccx(self, c1, c2, target):
        return InstructionSet([self._add(Instruction("ccx", 3), self._q(c1) + self._q(c2) + self._q(target))])

    def mcx(self, control_qubits, target_qubit):
        ctrls = self._q(control_qubits)
        tgt = self._q(target_qubit)
        name = {0: "x", 1: "cx", 2: "ccx"}.get(len(ctrls), "mcx")
        return InstructionSet([self._add(Instruction(name, len(ctrls) + 1), ctrls + tgt)])

    def measure(self, qubit, cbit):
        qs, cs = self._q(qubit), self._c(cbit)
        if len(qs) != len(cs):
            raise ValueError("measure: %d qubits but %d clbits" % (len(qs), len(cs)))
        return InstructionSet([self._add(Instruction("measure", 1, 1), [q], [c]) for q, c in zip(qs, cs)])

    def reset(self, qubit):
        """put ``qubit`` (or each of several) back in |0>"""
        return InstructionSet([self._add(Instruction("reset", 1), [q]) for q in self._q(qubit)])

    def if_test(self, condition):
        """``with qc.if_test((clbit or register, value)) as else_:`` -- the gates added inside run only in the shots in which
        the classical bit (or the register, as an integer) reads ``value``; ``with else_:`` afterwards holds what runs in the
        others.  One ``if_else`` operation (IfElseOp) is appended when the block closes."""
        if not (isinstance(condition, tuple) and len(condition) == 2):
            raise TypeError("if_test takes a (Clbit or classical register, value) pair")
        return _IfContext(self, condition)

    def barrier(self, *qargs):
        qs = self._q(qargs) if qargs else list(self.qubits)
        self._add(Instruction("barrier", len(qs)), qs)

    # ---- composition -----------------------------------------------------------------
    def to_instruction(self):
        return Instruction(self.name, self.num_qubits, self.num_clbits, [], self)

    to_gate = to_instruction

    def append(self, instruction, qargs=None, cargs=None):
        if isinstance(instruction, QuantumCircuit):
            instruction = instruction.to_instruction()
        qs = self._q(qargs or [])
        cs = self._c(cargs or [])
        if len(qs) != instruction.num_qubits:
            raise ValueError("instruction %s acts on %d qubits, %d given"
                             % (instruction.name, instruction.num_qubits, len(qs)))
        return self._add(instruction, qs, cs)

    def inverse(self):
        """same bits, name + '_dg', negated global phase, every operation inverted on its own in reverse
        order (qiskit.QuantumCircuit.inverse takes no arguments either)"""
        inv = QuantumCircuit(self.num_qubits, self.num_clbits, name=self.name + "_dg",
                             global_phase=-self.global_phase)
        for ci in reversed(self.data):
            qs = [inv.qubits[self._qindex[id(q)]] for q in ci.qubits]
            cs = [inv.clbits[self._cindex[id(c)]] for c in ci.clbits]
            inv._add(ci.operation.inverse(), qs, cs)
        return inv


def AND(num_variable_qubits, flags=None):
    """Counterpart of qiskit.circuit.library.AND(num_variable_qubits, flags) (QCMRF.py:9,225):
    a circuit on ``num_variable_qubits + 1`` qubits that XORs the conjunction of the flagged
    variables onto the last qubit.  flag > 0: variable as is; flag < 0: negated; 0: ignored."""
    flags = list(flags) if flags is not None else [1] * num_variable_qubits
    if len(flags) != num_variable_qubits:
        raise ValueError("AND: %d flags for %d variables" % (len(flags), num_variable_qubits))
    inner = QuantumCircuit(num_variable_qubits + 1, name="and")
    ctrl = [q for q, f in enumerate(flags) if f != 0]
    flip = [q for q, f in enumerate(flags) if f < 0]
    if flip:
        inner.x(flip)
    inner.mcx(ctrl, num_variable_qubits)
    if flip:
        inner.x(flip)
    # nested as Qiskit nests it: the AND circuit holds ONE gate "and" whose definition is x.. mcx x..
    circ = QuantumCircuit(num_variable_qubits + 1, name="and")
    circ.append(inner.to_gate(), list(range(num_variable_qubits + 1)))
    return circ
