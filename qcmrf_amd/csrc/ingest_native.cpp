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
// build_program(...), below it, is the back half of that front end: the fold's indexing, the layout and the encoded records.
#define PY_SSIZE_T_CLEAN
#include <Python.h>

#include <algorithm>
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

// ---- the back half: fold + plan + encode of a front-end circuit (qcmrf_amd/frontend.py, planner.py, program.py) -------------
//
//     build_program(num_qubits, opened, groups, shapes, n_shards, layout, global_phase)
//         -> (layout, records: bytearray of qsv_op, pool: bytearray of doubles, populated, n_ops)   or   None
//
// ``opened`` and ``groups`` are read_circuit's; ``shapes`` is a sequence of (k, m, c0), one entry per table shape: m the
// sandwiched 2x2 stack of the groups on k qubits in program order, complex128 (groups, 2^(k-1), 2, 2), and c0 its column 0
// times sqrt 2, complex128 (groups, 2^(k-1), 2).  No floating-point arithmetic happens here: entries are compared with 0 and
// 1 and copied.  What is done is the indexing of frontend.compile_blocks' fold, planner.plan for an op list of one init and
// diagonal factors (no dense target: no swap, no pass head, one layout) and program.encode for those ops.  The same
// contract as the walk: None means "not mine", and no exception leaves.

const int REC_MAX_CTRL = 16;                  // QSV_MAX_CTRL (include/qsv.h), _lib.MAX_CTRL
const int REC_OP_INIT_ZERO = 0, REC_OP_INIT_UNIFORM = 1, REC_OP_DIAG = 4;
const int PLAN_MULTI_R = 5, PLAN_LANE_BITS = 6, PLAN_GEN_TOP_MIN_L = 33, PLAN_REG_MIN_L = 14;   // planner.py

struct Record {                               // qsv_op (include/qsv.h), _lib.OP_DTYPE
    int32_t kind, target, n, flags;
    int32_t qubits[REC_MAX_CTRL], vals[REC_MAX_CTRL];
    uint64_t data_off, mask;
    double angle;
};
static_assert(sizeof(Record) == 168, "qsv_op is 168 bytes");
static_assert(MAX_GROUP_BITS <= REC_MAX_CTRL, "a factor of more qubits than a record holds is declined with its table shape");

struct Buf {                                  // a C-contiguous complex128 buffer of a given shape
    Py_buffer v;
    bool held = false;
    ~Buf()
    {
        if (held)
            PyBuffer_Release(&v);
    }
    Buf() {}
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    bool get(PyObject *o, int ndim, const Py_ssize_t *shape)
    {
        if (!PyObject_CheckBuffer(o) || PyObject_GetBuffer(o, &v, PyBUF_C_CONTIGUOUS | PyBUF_FORMAT) < 0)
            return false;
        held = true;
        if (!v.format || strcmp(v.format, "Zd") || v.itemsize != 16 || v.ndim != ndim || !v.shape || !v.buf)
            return false;
        for (int i = 0; i < ndim; i++)
            if (v.shape[i] != shape[i])
                return false;
        return true;
    }
    const double *at(Py_ssize_t element) const { return (const double *)v.buf + 2 * element; }
};

struct Factor {
    int n;                                    // qubits: the surviving selects, then the target
    int q[MAX_GROUP_BITS];
    int shape, row;                           // where its table is read: entry ``shape`` of shapes, group ``row`` of it
    int kept[MAX_GROUP_BITS];                 // the select index bits that survive
};

bool exact_index(PyObject *x, long limit, int &out)
{
    if (!PyLong_CheckExact(x))
        return false;
    long v = PyLong_AsLong(x);
    if (v < 0 || v >= limit)
        return false;                         // (-1 with an error set included: the caller clears it)
    out = (int)v;
    return true;
}

bool build_program_impl(PyObject *args, Ref &result)
{
    if (!PyTuple_CheckExact(args) || PyTuple_GET_SIZE(args) != 7)
        return false;
    PyObject *a_nq = PyTuple_GET_ITEM(args, 0), *a_opened = PyTuple_GET_ITEM(args, 1), *a_groups = PyTuple_GET_ITEM(args, 2);
    PyObject *a_shapes = PyTuple_GET_ITEM(args, 3), *a_shards = PyTuple_GET_ITEM(args, 4), *a_layout = PyTuple_GET_ITEM(args, 5);
    PyObject *a_phase = PyTuple_GET_ITEM(args, 6);

    if (!PyFloat_CheckExact(a_phase) || PyFloat_AS_DOUBLE(a_phase) != 0.0)
        return false;                         // a global phase rides in the first diagonal: backend._plan multiplies it in
    if (!PyUnicode_CheckExact(a_layout))
        return false;
    bool reference = is_name(a_layout, "reference");
    if (!reference && !is_name(a_layout, "auto"))
        return false;
    int nq = 0;
    if (!exact_index(a_nq, 65, nq) || nq < 1)
        return false;                         // the init mask is one 64-bit word
    if (!PyLong_CheckExact(a_shards))
        return false;
    long n_shards = PyLong_AsLong(a_shards);
    if (n_shards < 1 || (n_shards & (n_shards - 1)))
        return false;
    int g = 0;
    while ((1L << g) < n_shards)
        g++;
    int L = nq - g;
    if (L < 1)
        return false;

    // ---- the fold: which selects survive, which factors are the identity, what is populated afterwards ------------------
    if (!PyTuple_CheckExact(a_opened) || !PyList_CheckExact(a_groups))
        return false;
    uint64_t populated = 0;
    for (Py_ssize_t i = 0; i < PyTuple_GET_SIZE(a_opened); i++) {
        int q;
        if (!exact_index(PyTuple_GET_ITEM(a_opened, i), nq, q))
            return false;
        populated |= (uint64_t)1 << q;
    }
    Ref shapes(PySequence_Fast(a_shapes, "shapes"));
    if (!shapes.p)
        return false;
    Py_ssize_t n_shapes = PySequence_Fast_GET_SIZE(shapes.p), n_groups = PyList_GET_SIZE(a_groups);
    if (n_shapes > MAX_GROUP_BITS || n_groups < 1)
        return false;
    for (Py_ssize_t i = 0; i < n_groups; i++) {
        PyObject *grp = PyList_GET_ITEM(a_groups, i);
        if (!PyTuple_CheckExact(grp) || PyTuple_GET_SIZE(grp) != 6 || !PyTuple_CheckExact(PyTuple_GET_ITEM(grp, 1)))
            return false;
    }
    int shape_k[MAX_GROUP_BITS], shape_rows[MAX_GROUP_BITS], shape_seen[MAX_GROUP_BITS];
    Buf mats[MAX_GROUP_BITS], col0[MAX_GROUP_BITS];
    for (Py_ssize_t s = 0; s < n_shapes; s++) {
        PyObject *e = PySequence_Fast_GET_ITEM(shapes.p, s);
        if (!PyTuple_CheckExact(e) || PyTuple_GET_SIZE(e) != 3 || !exact_index(PyTuple_GET_ITEM(e, 0), MAX_GROUP_BITS + 1, shape_k[s]) ||
            shape_k[s] < 2)
            return false;
        for (Py_ssize_t t = 0; t < s; t++)
            if (shape_k[t] == shape_k[s])
                return false;
        Py_ssize_t rows = 0;
        for (Py_ssize_t i = 0; i < n_groups; i++)
            rows += PyTuple_GET_SIZE(PyTuple_GET_ITEM(PyList_GET_ITEM(a_groups, i), 1)) == shape_k[s];
        Py_ssize_t sm[4] = {rows, (Py_ssize_t)1 << (shape_k[s] - 1), 2, 2};
        if (rows < 1 || !mats[s].get(PyTuple_GET_ITEM(e, 1), 4, sm) || !col0[s].get(PyTuple_GET_ITEM(e, 2), 3, sm))
            return false;
        shape_rows[s] = (int)rows;
        shape_seen[s] = 0;
    }

    std::vector<Factor> factors;
    factors.reserve((size_t)n_groups);
    size_t pool_doubles = 0;
    for (Py_ssize_t i = 0; i < n_groups; i++) {
        PyObject *grp = PyList_GET_ITEM(a_groups, i), *glob = PyTuple_GET_ITEM(grp, 1);
        int k = (int)PyTuple_GET_SIZE(glob), s = 0, anc, sel[MAX_GROUP_BITS];
        while (s < n_shapes && shape_k[s] != k)
            s++;
        if (s == n_shapes || shape_seen[s] >= shape_rows[s] || !exact_index(PyTuple_GET_ITEM(grp, 0), nq, anc))
            return false;
        for (int j = 0; j < k; j++) {
            if (!exact_index(PyTuple_GET_ITEM(glob, j), nq, sel[j]))
                return false;
            for (int t = 0; t < j; t++)
                if (sel[t] == sel[j])
                    return false;
        }
        if (sel[k - 1] != anc)
            return false;                     // the target is the last qubit of its blocks
        Factor f;
        f.n = 0;
        f.shape = s;
        f.row = shape_seen[s]++;
        for (int e = 0; e + 1 < k; e++)
            if ((populated >> sel[e]) & 1) {  // a select on a qubit still |0> reads 0: its index bit is sliced away
                f.kept[f.n] = e;
                f.q[f.n++] = sel[e];
            }
        int ns = f.n;
        f.q[f.n++] = anc;
        // the identity writes nothing: an exact comparison of every surviving 2x2 with [[1, 0], [0, 1]]
        const double *m = mats[s].at((Py_ssize_t)f.row << (k + 1));
        bool identity = true;
        for (int j = 0; j < (1 << ns) && identity; j++) {
            int at = 0;
            for (int b = 0; b < ns; b++)
                at |= ((j >> b) & 1) << f.kept[b];
            const double *x = m + 8 * at;
            identity = x[0] == 1.0 && x[1] == 0.0 && x[2] == 0.0 && x[3] == 0.0 && x[4] == 0.0 && x[5] == 0.0 && x[6] == 1.0 && x[7] == 0.0;
        }
        if (identity)
            continue;
        pool_doubles += (size_t)4 << ns;
        factors.push_back(f);
        populated |= (uint64_t)1 << anc;
    }

    // ---- planner.choose_layout: no op has a dense target, so no qubit is ever exchanged and one layout holds throughout -----
    int lay[64];
    if (reference) {
        for (int q = 0; q < nq; q++)
            lay[q] = q;
    } else {
        auto uniform = [&](int q) { return (int)((populated >> q) & 1); };
        // shard bits: never-dense qubits in uniform superposition first, the highest index first among equals
        bool shard[64] = {false};
        int rank[64];
        for (int q = 0; q < nq; q++)
            rank[q] = q;
        std::stable_sort(rank, rank + nq, [&](int a, int b) {
            if (uniform(a) != uniform(b))
                return uniform(a) > uniform(b);
            return a > b;
        });
        for (int i = 0; i < g; i++)
            shard[rank[i]] = true;
        std::vector<int> quiet_u, quiet_z;
        for (int q = 0; q < nq; q++)
            if (!shard[q])
                (uniform(q) ? quiet_u : quiet_z).push_back(q);
        if (L >= PLAN_REG_MIN_L) {
            // the generator's register bits go to the qubits the fewest factors touch
            int uses[64] = {0};
            for (const Factor &f : factors)
                for (int j = 0; j < f.n; j++)
                    uses[f.q[j]]++;           // (shard qubits are counted and never looked at)
            std::vector<int> cand(quiet_u);
            cand.insert(cand.end(), quiet_z.begin(), quiet_z.end());
            std::stable_sort(cand.begin(), cand.end(), [&](int a, int b) {
                if (uses[a] != uses[b])
                    return uses[a] < uses[b];
                return a > b;
            });
            std::vector<int> regq(cand.begin(), cand.begin() + (cand.size() < (size_t)PLAN_MULTI_R ? cand.size() : (size_t)PLAN_MULTI_R));
            std::stable_sort(regq.begin(), regq.end(), [&](int a, int b) {
                if (uses[a] != uses[b])
                    return uses[a] > uses[b];
                return a < b;
            });
            if (cand.size() - regq.size() >= (size_t)PLAN_LANE_BITS) {
                bool is_reg[64] = {false};
                for (int q : regq)
                    is_reg[q] = true;
                std::vector<int> others, zeros;
                for (int q : quiet_u)
                    if (!is_reg[q])
                        others.push_back(q);
                for (int q : quiet_z)
                    if (!is_reg[q])
                        zeros.push_back(q);
                if (L >= PLAN_GEN_TOP_MIN_L) {
                    zeros.insert(zeros.end(), regq.begin(), regq.end());      // highest local positions, fewest uses on top
                    quiet_u.swap(others);
                } else {
                    size_t low = others.size() < (size_t)PLAN_LANE_BITS ? others.size() : (size_t)PLAN_LANE_BITS;
                    quiet_u.assign(others.begin(), others.begin() + low);
                    quiet_u.insert(quiet_u.end(), regq.begin(), regq.end());
                    quiet_u.insert(quiet_u.end(), others.begin() + low, others.end());
                }
                quiet_z.swap(zeros);
            }
        }
        int p = 0;
        for (int q : quiet_u)
            lay[q] = p++;
        for (int q : quiet_z)
            lay[q] = p++;
        if (p != L)
            return false;
        for (int q = 0; q < nq; q++)
            if (shard[q])
                lay[q] = p++;                 // shard qubits in ascending order on the bits above the local ones
    }

    // ---- program.encode of [init] + the remapped factors; the tables in op order, transposed to (target value, select) -----
    size_t n_ops = 1 + factors.size();
    Ref rec(PyByteArray_FromStringAndSize(nullptr, (Py_ssize_t)(n_ops * sizeof(Record))));
    Ref pool(PyByteArray_FromStringAndSize(nullptr, (Py_ssize_t)(pool_doubles * sizeof(double))));
    if (!rec.p || !pool.p)
        return false;
    char *rp = PyByteArray_AS_STRING(rec.p);
    double *pp = (double *)PyByteArray_AS_STRING(pool.p);
    memset(rp, 0, n_ops * sizeof(Record));
    Record r;
    memset(&r, 0, sizeof r);
    for (int q = 0; q < nq; q++)
        if ((populated >> q) & 1)
            r.mask |= (uint64_t)1 << lay[q];
    r.kind = r.mask ? REC_OP_INIT_UNIFORM : REC_OP_INIT_ZERO;
    memcpy(rp, &r, sizeof r);
    size_t top = 0;
    for (size_t i = 0; i < factors.size(); i++) {
        const Factor &f = factors[i];
        int ns = f.n - 1, k = shape_k[f.shape];
        memset(&r, 0, sizeof r);
        r.kind = REC_OP_DIAG;
        r.n = f.n;
        for (int j = 0; j < f.n; j++)
            r.qubits[j] = lay[f.q[j]];
        r.data_off = top;
        memcpy(rp + (i + 1) * sizeof(Record), &r, sizeof r);
        const double *c = col0[f.shape].at((Py_ssize_t)f.row << k);
        for (int row = 0; row < 2; row++)
            for (int j = 0; j < (1 << ns); j++) {
                int at = 0;
                for (int b = 0; b < ns; b++)
                    at |= ((j >> b) & 1) << f.kept[b];
                memcpy(pp + top, c + 4 * at + 2 * row, 2 * sizeof(double));
                top += 2;
            }
    }
    if (top != pool_doubles)
        return false;
    Ref layout(int_tuple(lay, nq));
    if (!layout.p)
        return false;
    Ref out(Py_BuildValue("(OOOKn)", layout.p, rec.p, pool.p, (unsigned long long)populated, (Py_ssize_t)n_ops));
    if (!out.p)
        return false;
    result.take(out);
    return true;
}

PyObject *build_program(PyObject *, PyObject *args)
{
    Ref result;
    if (build_program_impl(args, result))
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
    {"build_program", build_program, METH_VARARGS,
     "build_program(num_qubits, opened, groups, shapes, n_shards, layout, global_phase) -> (layout, qsv_op records, data pool, populated, "
     "number of ops) of a circuit read_circuit described, shapes being (k, 2x2 stack, its column 0 times sqrt 2) per table shape, or None (not mine)"},
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
