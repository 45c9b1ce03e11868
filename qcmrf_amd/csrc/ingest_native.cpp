// Native reader of the structural signature of a clique block (host code, CPython C API; no HIP).
//
// qcmrf_amd/ingest.py recognises a ``cU_C`` / ``cU_C_dg`` definition -- nothing but AND . cp . AND triples -- by a
// signature it reads off the objects: gate names, qubit positions, and the signatures of the AND definitions.  The
// reading is attribute access and tuple building and nothing else, and it is most of the host time of a step.  This
// module does the same reads through the C API and returns exactly what the Python code builds:
//
//     read_block(definition) -> ((names, lens, pos, and_keys), [cp angles as floats])   or   None
//
// with and_keys[k] = (names, pos, ctrl_state) of the unwrapped AND at instruction k and None at the cp positions.
// The tuples compare equal to the Python ones, so both paths share the memo tables keyed on them.
//
// The reader decides nothing.  None means "not mine": any shape off the fast path (legacy tuple instructions, bits that
// are not the definition's own objects, an attribute that raises, a parameter that does not convert, a global phase,
// a count that is no multiple of 3, ...) is left to the Python code, which then takes its decision or raises its error.
// No exception ever leaves this module.
//
// read_circuit(circuit), further down, is the front end's walk over a whole circuit of the reference's construction
// (qcmrf_amd/frontend.py): it calls the reader's code directly for every composite and follows the same contract.
#define PY_SSIZE_T_CLEAN
#include <Python.h>

#include <cstdint>
#include <cstring>
#include <vector>

namespace {

PyObject *s_data, *s_qubits, *s_operation, *s_name, *s_condition, *s_definition, *s_global_phase, *s_ctrl_state, *s_params, *s_clbits;
PyObject *g_primitives;                       // ingest._PRIMITIVES: names that are never opened (set_primitives)
PyObject *g_block_of_key;                     // ingest._block_of_key: signature -> block, memoised there (set_block_of_key)

const int MAX_BITS = 64;                      // qubits of one definition (the engine itself stops at far fewer)
const int MAX_AND_OPS = 33;                   // as ingest._and_key
const int MAX_AND_POS = 256;

struct Ref {                                  // one owned reference
    PyObject *p;
    explicit Ref(PyObject *q = nullptr) : p(q) {}
    ~Ref() { Py_XDECREF(p); }
    Ref(const Ref &) = delete;
    Ref &operator=(const Ref &) = delete;
    void take(Ref &o) { PyObject *old = p; p = o.p; o.p = nullptr; Py_XDECREF(old); }
    PyObject *release() { PyObject *q = p; p = nullptr; return q; }
};

// getattr(o, name, None): a new reference; nullptr (error left set) when the attribute raises anything else
// (a plain miss builds no exception object: the in-tree container's gates have no ``ctrl_state``, Qiskit 2's no ``condition``)
PyObject *attr_opt(PyObject *o, PyObject *name)
{
    PyObject *v = nullptr;
#if PY_VERSION_HEX >= 0x030D0000
    int found = PyObject_GetOptionalAttr(o, name, &v);
#else
    int found = _PyObject_LookupAttr(o, name, &v);
#endif
    if (found < 0)
        return nullptr;
    if (found)
        return v;
    Py_RETURN_NONE;
}

// what iterating ``o`` yields, as a list or tuple (new reference)
PyObject *fast_seq(PyObject *o)
{
    if (PyList_CheckExact(o) || PyTuple_CheckExact(o)) {
        Py_INCREF(o);
        return o;
    }
    return PySequence_List(o);
}

// bool(getattr(definition, "global_phase", 0)): 1 / 0, -1 if it raises
int has_phase(PyObject *definition)
{
    Ref g(attr_opt(definition, s_global_phase));
    if (!g.p)
        return -1;
    return g.p == Py_None ? 0 : PyObject_IsTrue(g.p);
}

struct Bits {                                 // position of a bit by object identity; the last of equal pointers, as a dict would keep
    PyObject *b[MAX_BITS];
    Py_ssize_t n;
    bool fill(PyObject *seq)
    {
        n = PySequence_Fast_GET_SIZE(seq);
        if (n > MAX_BITS)
            return false;
        PyObject **it = PySequence_Fast_ITEMS(seq);
        for (Py_ssize_t i = 0; i < n; i++)
            b[i] = it[i];
        return true;
    }
    long find(PyObject *q) const
    {
        for (Py_ssize_t i = n; i-- > 0;)
            if (b[i] == q)
                return (long)i;
        return -1;
    }
};

PyObject *int_tuple(const int *v, Py_ssize_t n)
{
    PyObject *t = PyTuple_New(n);
    if (!t)
        return nullptr;
    for (Py_ssize_t i = 0; i < n; i++) {
        PyObject *x = PyLong_FromLong(v[i]);
        if (!x) {
            Py_DECREF(t);
            return nullptr;
        }
        PyTuple_SET_ITEM(t, i, x);
    }
    return t;
}

// ingest._and_key after ingest._unwrap: (names, pos, ctrl_state) into ``key``; false: not mine
bool read_and_key(PyObject *definition_in, Ref &key)
{
    Py_INCREF(definition_in);
    Ref definition(definition_in);
    for (int level = 0; level < 8; level++) {
        Ref data(PyObject_GetAttr(definition.p, s_data));
        if (!data.p)
            return false;
        Ref seq(fast_seq(data.p));
        if (!seq.p)
            return false;
        if (PySequence_Fast_GET_SIZE(seq.p) != 1)
            break;
        PyObject *ci = PySequence_Fast_GET_ITEM(seq.p, 0);
        Ref op(PyObject_GetAttr(ci, s_operation));
        if (!op.p)
            return false;
        Ref qargs(PyObject_GetAttr(ci, s_qubits));
        if (!qargs.p)
            return false;
        Ref name(PyObject_GetAttr(op.p, s_name));
        if (!name.p || !PyUnicode_CheckExact(name.p))
            return false;
        int prim = PyDict_Contains(g_primitives, name.p);
        if (prim < 0)
            return false;
        if (prim)
            break;
        Ref cond(attr_opt(op.p, s_condition));
        if (!cond.p)
            return false;
        if (cond.p != Py_None)
            break;
        Ref inner(attr_opt(op.p, s_definition));
        if (!inner.p)
            return false;
        if (inner.p == Py_None)
            break;
        int ph = has_phase(definition.p);
        if (ph < 0)
            return false;
        if (ph)
            break;
        Ref own(PyObject_GetAttr(definition.p, s_qubits));
        if (!own.p)
            return false;
        Ref a(fast_seq(qargs.p)), b(fast_seq(own.p));
        if (!a.p || !b.p)
            return false;
        Py_ssize_t na = PySequence_Fast_GET_SIZE(a.p);
        if (na != PySequence_Fast_GET_SIZE(b.p))
            break;
        PyObject **ia = PySequence_Fast_ITEMS(a.p), **ib = PySequence_Fast_ITEMS(b.p);
        for (Py_ssize_t i = 0; i < na; i++)
            if (ia[i] != ib[i])
                return false;                 // equal or not is for Bit.__eq__ to say
        definition.take(inner);
    }

    Ref data(PyObject_GetAttr(definition.p, s_data));
    if (!data.p)
        return false;
    Ref seq(fast_seq(data.p));
    if (!seq.p)
        return false;
    Py_ssize_t n = PySequence_Fast_GET_SIZE(seq.p);
    if (!(n & 1) || n > MAX_AND_OPS || has_phase(definition.p) != 0)
        return false;
    Ref qs(attr_opt(definition.p, s_qubits));
    if (!qs.p || qs.p == Py_None)
        return false;
    Ref qseq(fast_seq(qs.p));
    Bits bits;
    if (!qseq.p || !bits.fill(qseq.p))
        return false;

    Ref names(PyTuple_New(n));
    if (!names.p)
        return false;
    int pos[MAX_AND_POS];
    Py_ssize_t npos = 0;
    Ref state;
    for (Py_ssize_t k = 0; k < n; k++) {
        PyObject *ci = PySequence_Fast_GET_ITEM(seq.p, k);
        Ref op(PyObject_GetAttr(ci, s_operation));
        if (!op.p)
            return false;
        Ref qargs(PyObject_GetAttr(ci, s_qubits));
        if (!qargs.p)
            return false;
        Ref cond(attr_opt(op.p, s_condition));
        if (!cond.p)
            return false;
        if (cond.p != Py_None && PyObject_IsTrue(cond.p) != 0)
            return false;
        Ref qa(fast_seq(qargs.p));
        if (!qa.p)
            return false;
        Py_ssize_t nq = PySequence_Fast_GET_SIZE(qa.p);
        if (npos + nq > MAX_AND_POS)
            return false;
        PyObject **iq = PySequence_Fast_ITEMS(qa.p);
        for (Py_ssize_t j = 0; j < nq; j++) {
            long at = bits.find(iq[j]);
            if (at < 0)
                return false;
            pos[npos++] = (int)at;
        }
        PyObject *name = PyObject_GetAttr(op.p, s_name);
        if (!name)
            return false;
        PyTuple_SET_ITEM(names.p, k, name);   // the tuple owns it from here
        if (!PyUnicode_CheckExact(name))
            return false;
        if (k == n >> 1) {
            Ref st(attr_opt(op.p, s_ctrl_state));
            if (!st.p || (st.p != Py_None && !PyLong_CheckExact(st.p)))
                return false;
            state.take(st);
        }
    }
    Ref p(int_tuple(pos, npos));
    if (!p.p)
        return false;
    PyObject *t = PyTuple_New(3);
    if (!t)
        return false;
    PyTuple_SET_ITEM(t, 0, names.release());
    PyTuple_SET_ITEM(t, 1, p.release());
    PyTuple_SET_ITEM(t, 2, state.release());
    Ref done(t);
    key.take(done);
    return true;
}

// what ingest._emit_phase_block reads before its table lookup; false: not mine
bool read_block_impl(PyObject *definition, Ref &result)
{
    Ref data(PyObject_GetAttr(definition, s_data));
    if (!data.p)
        return false;
    Ref seq(fast_seq(data.p));
    if (!seq.p)
        return false;
    Py_ssize_t n = PySequence_Fast_GET_SIZE(seq.p);
    if (n < 3 || n % 3 || has_phase(definition) != 0)
        return false;
    Ref qs(attr_opt(definition, s_qubits));
    if (!qs.p || qs.p == Py_None)
        return false;
    Ref qseq(fast_seq(qs.p));
    Bits bits;
    if (!qseq.p || !bits.fill(qseq.p))
        return false;

    Ref names(PyTuple_New(n)), lens(PyTuple_New(n)), and_keys(PyTuple_New(n)), angles(PyList_New(0));
    if (!names.p || !lens.p || !and_keys.p || !angles.p)
        return false;
    std::vector<int> pos;
    pos.reserve(128);
    for (Py_ssize_t k = 0; k < n; k++) {
        PyObject *ci = PySequence_Fast_GET_ITEM(seq.p, k);
        Ref op(PyObject_GetAttr(ci, s_operation));
        if (!op.p)
            return false;
        Ref qargs(PyObject_GetAttr(ci, s_qubits));
        if (!qargs.p)
            return false;
        PyObject *name = PyObject_GetAttr(op.p, s_name);
        if (!name)
            return false;
        PyTuple_SET_ITEM(names.p, k, name);
        if (!PyUnicode_CheckExact(name))
            return false;
        Ref qa(fast_seq(qargs.p));
        if (!qa.p)
            return false;
        Py_ssize_t nq = PySequence_Fast_GET_SIZE(qa.p);
        PyObject **iq = PySequence_Fast_ITEMS(qa.p);
        for (Py_ssize_t j = 0; j < nq; j++) {
            long at = bits.find(iq[j]);
            if (at < 0)
                return false;
            pos.push_back((int)at);
        }
        PyObject *ln = PyLong_FromSsize_t(nq);
        if (!ln)
            return false;
        PyTuple_SET_ITEM(lens.p, k, ln);

        Ref cond(attr_opt(op.p, s_condition));
        if (!cond.p)
            return false;
        if (k % 3 == 1) {
            // the phase gate: unconditioned, closed control, every parameter a float or convertible to one
            if (cond.p != Py_None)
                return false;
            Ref st(attr_opt(op.p, s_ctrl_state));
            if (!st.p)
                return false;
            if (st.p != Py_None && !(PyLong_CheckExact(st.p) && PyLong_AsLong(st.p) == 1))
                return false;
            Ref params(PyObject_GetAttr(op.p, s_params));
            if (!params.p || PyObject_IsTrue(params.p) != 1)
                return false;
            Ref ps(fast_seq(params.p));
            if (!ps.p)
                return false;
            Py_ssize_t np = PySequence_Fast_GET_SIZE(ps.p);
            if (np < 1)
                return false;
            PyObject **ip = PySequence_Fast_ITEMS(ps.p);
            for (Py_ssize_t j = 0; j < np; j++) {
                Ref f;
                if (PyFloat_CheckExact(ip[j])) {
                    Py_INCREF(ip[j]);
                    Ref same(ip[j]);
                    f.take(same);
                } else {
                    Ref conv(PyObject_CallFunctionObjArgs((PyObject *)&PyFloat_Type, ip[j], nullptr));
                    if (!conv.p)
                        return false;
                    f.take(conv);
                }
                if (j == 0 && PyList_Append(angles.p, f.p) < 0)
                    return false;
            }
            Py_INCREF(Py_None);
            PyTuple_SET_ITEM(and_keys.p, k, Py_None);
        } else {
            // an AND, compute or uncompute: every one is a distinct object and is read afresh
            if (cond.p != Py_None && PyObject_IsTrue(cond.p) != 0)
                return false;
            Ref inner(attr_opt(op.p, s_definition));
            if (!inner.p || inner.p == Py_None)
                return false;
            Ref key;
            if (!read_and_key(inner.p, key))
                return false;
            PyTuple_SET_ITEM(and_keys.p, k, key.release());
        }
    }
    Ref p(int_tuple(pos.data(), (Py_ssize_t)pos.size()));
    if (!p.p)
        return false;
    PyObject *key = PyTuple_New(4);
    if (!key)
        return false;
    PyTuple_SET_ITEM(key, 0, names.release());
    PyTuple_SET_ITEM(key, 1, lens.release());
    PyTuple_SET_ITEM(key, 2, p.release());
    PyTuple_SET_ITEM(key, 3, and_keys.release());
    Ref k(key);
    PyObject *out = PyTuple_New(2);
    if (!out)
        return false;
    PyTuple_SET_ITEM(out, 0, k.release());
    PyTuple_SET_ITEM(out, 1, angles.release());
    Ref done(out);
    result.take(done);
    return true;
}

// ---- the front end: one walk over a circuit of the reference's construction (qcmrf_amd/frontend.py) -------------------------
//
//     read_circuit(circuit) -> (num_qubits, num_clbits, opened wires, groups, [(clbit, qubit)], source gates)   or   None
//
// with one group = (ancilla, global qubits of its blocks, block of B, angles of B, block of B', angles of B'), a block being
// what ingest._block_of_key answers for the signature read_block reads.  The grammar and why each condition is there:
// DESIGN.md 4.  Like read_block it decides nothing: everything off the grammar is None, and the Python pipeline
// (ingest + passes.optimise) then takes its decision or raises its error.

enum { W_OPENED = 1, W_ANCILLA = 2, W_USED = 4, W_MEASURED = 8 };

struct PtrMap {                               // bit object -> index by identity; the last of equal pointers, as a dict would keep
    std::vector<PyObject *> keys;
    std::vector<int> vals;
    size_t mask;
    static size_t hash(PyObject *p) { return (size_t)(((uintptr_t)p >> 4) * (uintptr_t)0x9E3779B97F4A7C15ull >> 20); }
    void build(PyObject **items, Py_ssize_t n)
    {
        size_t cap = 16;
        while (cap < (size_t)n * 4)
            cap <<= 1;
        keys.assign(cap, nullptr);
        vals.assign(cap, -1);
        mask = cap - 1;
        for (Py_ssize_t i = 0; i < n; i++) {
            size_t at = hash(items[i]) & mask;
            while (keys[at] && keys[at] != items[i])
                at = (at + 1) & mask;
            keys[at] = items[i];
            vals[at] = (int)i;
        }
    }
    int find(PyObject *p) const
    {
        size_t at = hash(p) & mask;
        while (keys[at]) {
            if (keys[at] == p)
                return vals[at];
            at = (at + 1) & mask;
        }
        return -1;
    }
};

const int MAX_GROUP_BITS = 9;                 // passes.fuse_sandwich takes tables of 2 .. 9 qubits
const Py_ssize_t MAX_WIRES = 1 << 16;

bool is_name(PyObject *name, const char *text) { return PyUnicode_CompareWithASCIIString(name, text) == 0; }

// the global qubits (controls..., scratch, other) of a block on the instruction qubits ``q``; false: not mine
bool block_wires(PyObject *blk, const std::vector<int> &q, int *glob, int &k, long &n_src)
{
    if (!PyTuple_CheckExact(blk) || PyTuple_GET_SIZE(blk) != 5)
        return false;
    PyObject *ctrls = PyTuple_GET_ITEM(blk, 0);
    if (!PyList_CheckExact(ctrls) || PyList_GET_SIZE(ctrls) + 2 > MAX_GROUP_BITS)
        return false;
    k = 0;
    for (Py_ssize_t i = 0; i < PyList_GET_SIZE(ctrls) + 2; i++) {
        PyObject *x = i < PyList_GET_SIZE(ctrls) ? PyList_GET_ITEM(ctrls, i) : PyTuple_GET_ITEM(blk, 1 + (i - PyList_GET_SIZE(ctrls)));
        if (!PyLong_CheckExact(x))
            return false;
        long at = PyLong_AsLong(x);
        if (at < 0 || (size_t)at >= q.size())
            return false;
        for (int j = 0; j < k; j++)
            if (glob[j] == q[at])
                return false;
        glob[k++] = q[at];
    }
    PyObject *n = PyTuple_GET_ITEM(blk, 4);
    if (!PyLong_CheckExact(n))
        return false;
    n_src = PyLong_AsLong(n);
    return n_src >= 0;
}

bool read_circuit_impl(PyObject *circuit, Ref &result)
{
    Ref data(PyObject_GetAttr(circuit, s_data));
    if (!data.p)
        return false;
    Ref seq(fast_seq(data.p));
    if (!seq.p)
        return false;
    Ref qs(attr_opt(circuit, s_qubits)), cs(attr_opt(circuit, s_clbits));
    if (!qs.p || qs.p == Py_None || !cs.p || cs.p == Py_None)
        return false;
    Ref qseq(fast_seq(qs.p)), cseq(fast_seq(cs.p));
    if (!qseq.p || !cseq.p)
        return false;
    Py_ssize_t nq = PySequence_Fast_GET_SIZE(qseq.p), nc = PySequence_Fast_GET_SIZE(cseq.p);
    if (nq > MAX_WIRES || nc > MAX_WIRES)
        return false;
    PtrMap qmap, cmap;
    qmap.build(PySequence_Fast_ITEMS(qseq.p), nq);
    cmap.build(PySequence_Fast_ITEMS(cseq.p), nc);

    std::vector<unsigned char> wire((size_t)nq, 0);
    std::vector<int> opened, q;
    Ref groups(PyList_New(0)), measures(PyList_New(0));
    if (!groups.p || !measures.p)
        return false;
    long n_src = 0;
    int stage = 0;                            // of the group h a . B . x a . B' . x a . h a: gate tokens taken after the h
    int anc = -1, last_h = -1;                // last_h: the wire the gate token just before opened with h, else -1
    int glob[MAX_GROUP_BITS], k = 0;
    Ref blk1, lam1, blk2, lam2;

    Py_ssize_t n = PySequence_Fast_GET_SIZE(seq.p);
    for (Py_ssize_t at = 0; at < n; at++) {
        PyObject *ci = PySequence_Fast_GET_ITEM(seq.p, at);
        Ref op(PyObject_GetAttr(ci, s_operation));            // (a legacy tuple instruction has none: not mine)
        if (!op.p)
            return false;
        Ref qargs(PyObject_GetAttr(ci, s_qubits));
        if (!qargs.p)
            return false;
        Ref name(PyObject_GetAttr(op.p, s_name));
        if (!name.p || !PyUnicode_CheckExact(name.p))
            return false;
        Ref cond(attr_opt(op.p, s_condition));
        if (!cond.p || cond.p != Py_None)
            return false;
        Ref qa(fast_seq(qargs.p));
        if (!qa.p)
            return false;
        Py_ssize_t na = PySequence_Fast_GET_SIZE(qa.p);
        PyObject **iq = PySequence_Fast_ITEMS(qa.p);
        q.clear();
        for (Py_ssize_t j = 0; j < na; j++) {
            int w = qmap.find(iq[j]);
            if (w < 0)
                return false;                 // equal to a qubit of the circuit or not is for find_bit to say
            q.push_back(w);
        }
        if (is_name(name.p, "barrier") || is_name(name.p, "delay"))
            continue;
        if (is_name(name.p, "measure")) {
            Ref cargs(PyObject_GetAttr(ci, s_clbits));
            if (!cargs.p)
                return false;
            Ref ca(fast_seq(cargs.p));
            if (!ca.p || PySequence_Fast_GET_SIZE(ca.p) != 1 || na != 1)
                return false;
            int c = cmap.find(PySequence_Fast_GET_ITEM(ca.p, 0));
            if (c < 0)
                return false;
            Ref pair(Py_BuildValue("(ii)", c, q[0]));
            if (!pair.p || PyList_Append(measures.p, pair.p) < 0)
                return false;
            wire[q[0]] |= W_MEASURED;
            n_src++;
            continue;
        }
        for (int w : q)
            if (wire[w] & W_MEASURED)
                return false;                 // a gate after a measure on its qubit: the walk names it
        if (is_name(name.p, "h")) {
            if (na != 1)
                return false;
            int w = q[0];
            if (stage == 4 && w == anc) {
                Ref g(Py_BuildValue("(iNOOOO)", anc, int_tuple(glob, k), blk1.p, lam1.p, blk2.p, lam2.p));
                if (!g.p || PyList_Append(groups.p, g.p) < 0)
                    return false;
                stage = 0;
                last_h = -1;
            } else if (stage == 0 && wire[w] == 0) {
                wire[w] = W_OPENED;           // the first touch of its wire
                opened.push_back(w);
                last_h = w;
            } else {
                return false;
            }
            n_src++;
            continue;
        }
        if (is_name(name.p, "x")) {
            if (na != 1 || (stage != 1 && stage != 3) || q[0] != anc)
                return false;
            stage++;
            n_src++;
            continue;
        }
        // a composite: B of a group that the h just before opened, or its B'
        int prim = PyDict_Contains(g_primitives, name.p);
        const char *text = PyUnicode_AsUTF8(name.p);
        if (prim != 0 || !text || !strcmp(text, "reset") || strstr(text, "_o"))
            return false;                     // (``ccx_o1`` and its like are primitives under another name)
        if (stage != 0 && stage != 2)
            return false;
        Ref definition(attr_opt(op.p, s_definition));
        if (!definition.p || definition.p == Py_None)
            return false;
        Ref got;
        if (!read_block_impl(definition.p, got))
            return false;
        Ref blk(PyObject_CallFunctionObjArgs(g_block_of_key, PyTuple_GET_ITEM(got.p, 0), nullptr));
        if (!blk.p || blk.p == Py_None)
            return false;
        int here[MAX_GROUP_BITS], kh = 0;
        long src = 0;
        if (!block_wires(blk.p, q, here, kh, src))
            return false;
        PyObject *angles = PyTuple_GET_ITEM(got.p, 1);
        Py_INCREF(angles);
        Ref lam(angles);
        if (stage == 0) {
            if (last_h < 0 || here[kh - 1] != last_h)
                return false;                 // the ancilla is first touched by the h of its group
            for (int j = 0; j + 2 < kh; j++)
                if (wire[here[j]] & W_ANCILLA)
                    return false;             // nothing touches an ancilla after its group
            if (wire[here[kh - 2]] & (W_OPENED | W_ANCILLA))
                return false;                 // the scratch wire is never populated
            anc = last_h;
            opened.pop_back();
            wire[anc] = W_ANCILLA;
            for (int j = 0; j + 1 < kh; j++)
                wire[here[j]] |= W_USED;
            k = kh;
            for (int j = 0; j < kh; j++)
                glob[j] = here[j];
            blk1.take(blk);
            lam1.take(lam);
            stage = 1;
        } else {
            if (kh != k)
                return false;
            for (int j = 0; j < k; j++)
                if (here[j] != glob[j])
                    return false;             // both blocks on one qubit tuple
            blk2.take(blk);
            lam2.take(lam);
            stage = 3;
        }
        last_h = -1;
        n_src += src;
    }
    if (stage != 0 || PyList_GET_SIZE(groups.p) == 0 || opened.empty())
        return false;
    Ref op_t(int_tuple(opened.data(), (Py_ssize_t)opened.size()));
    if (!op_t.p)
        return false;
    Ref out(Py_BuildValue("(nnOOOl)", nq, nc, op_t.p, groups.p, measures.p, n_src));
    if (!out.p)
        return false;
    result.take(out);
    return true;
}

PyObject *read_circuit(PyObject *, PyObject *circuit)
{
    Ref result;
    if (g_primitives && g_block_of_key && read_circuit_impl(circuit, result))
        return result.release();
    PyErr_Clear();
    Py_RETURN_NONE;
}

PyObject *set_block_of_key(PyObject *, PyObject *fn)
{
    if (!PyCallable_Check(fn)) {
        PyErr_SetString(PyExc_TypeError, "set_block_of_key() takes ingest._block_of_key");
        return nullptr;
    }
    Py_INCREF(fn);
    Py_XSETREF(g_block_of_key, fn);
    Py_RETURN_NONE;
}

PyObject *read_block(PyObject *, PyObject *definition)
{
    Ref result;
    if (g_primitives && read_block_impl(definition, result))
        return result.release();
    PyErr_Clear();
    Py_RETURN_NONE;
}

PyObject *set_primitives(PyObject *, PyObject *names)
{
    if (!PyDict_Check(names)) {
        PyErr_SetString(PyExc_TypeError, "set_primitives() takes the dict of primitive gate names");
        return nullptr;
    }
    Py_INCREF(names);
    Py_XSETREF(g_primitives, names);
    Py_RETURN_NONE;
}

PyMethodDef methods[] = {
    {"read_block", read_block, METH_O,
     "read_block(definition) -> ((names, lens, pos, and_keys), [cp angles]) as ingest._emit_phase_block reads them, or None (not mine)"},
    {"set_primitives", set_primitives, METH_O, "set_primitives(dict): gate names whose definitions are never opened"},
    {"read_circuit", read_circuit, METH_O,
     "read_circuit(circuit) -> (num_qubits, num_clbits, opened wires, groups, [(clbit, qubit)], source gates) of a circuit of h openings and "
     "extraction groups, or None (not mine)"},
    {"set_block_of_key", set_block_of_key, METH_O, "set_block_of_key(callable): ingest._block_of_key"},
    {nullptr, nullptr, 0, nullptr}};

PyModuleDef module = {PyModuleDef_HEAD_INIT, "_ingest_native", "native reader of clique-block signatures (qcmrf_amd.ingest)", -1, methods,
                      nullptr, nullptr, nullptr, nullptr};

}  // namespace

PyMODINIT_FUNC PyInit__ingest_native(void)
{
    static const struct {
        PyObject **slot;
        const char *text;
    } strings[] = {{&s_data, "data"}, {&s_qubits, "qubits"}, {&s_operation, "operation"}, {&s_name, "name"}, {&s_condition, "condition"},
                   {&s_definition, "definition"}, {&s_global_phase, "global_phase"}, {&s_ctrl_state, "ctrl_state"}, {&s_params, "params"}, {&s_clbits, "clbits"}};
    for (const auto &s : strings) {
        if (!*s.slot)
            *s.slot = PyUnicode_InternFromString(s.text);
        if (!*s.slot)
            return nullptr;
    }
    return PyModule_Create(&module);
}
