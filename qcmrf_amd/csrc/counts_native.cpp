// Native counting and key formatting of sampled words (host code, CPython C API; no HIP).
//
// qcmrf_amd/backend.py turns the words a draw returns into Qiskit's count dict with np.unique and _format_keys: a sort,
// a bit matrix, and -- with more than one classical register -- a Python join per key.  This module does the same in
// one call and returns exactly the dict the Python code builds, keys, values and insertion order:
//
//     counts_dict(words, weights, num_clbits, creg_sizes) -> {bitstring: int}   or   None
//
//     words       contiguous uint64 buffer                       weights   None, or a contiguous int64 buffer of the same length
//     == _format_keys(*np.unique(words, return_counts=True), num_clbits, creg_sizes)                      (weights None)
//     == _format_keys(uv, [sum of the weights of the words equal to uv[i]], num_clbits, creg_sizes)       (weights given)
//
// Unsigned ascending order; keys num_clbits wide (at least 1), most significant bit first; with more than one register
// one group per register, last register first, joined by one space; values are Python ints.
//
// The module decides nothing.  None means "not mine": object arrays, strided or wrongly typed buffers, num_clbits past
// 64, words with a bit at or above the key width, register lists that are not (name, size >= 1) pairs adding up to
// num_clbits, an allocation that fails -- all are left to the Python code.  No exception ever leaves this module.
#define PY_SSIZE_T_CLEAN
#include <Python.h>

#include <cstdint>
#include <cstdlib>
#include <cstring>

namespace {

const int MAX_DIGIT = 11;                     // radix-sort digit at most: 4 passes of 9 bits at 34, 6 of 11 at 64; an 8 KiB histogram

struct View {                                 // a buffer view that is released on every path
    Py_buffer b;
    bool held = false;
    ~View() { if (held) PyBuffer_Release(&b); }
    // contiguous, one-dimensional, 8-byte items of one of the two format characters: true; anything else false, no error left
    bool get(PyObject *o, char c0, char c1)
    {
        if (PyObject_GetBuffer(o, &b, PyBUF_FORMAT | PyBUF_STRIDES) < 0) {
            PyErr_Clear();
            return false;
        }
        held = true;
        if (b.ndim != 1 || b.itemsize != 8 || !b.format || !PyBuffer_IsContiguous(&b, 'C'))
            return false;
        const char *f = b.format;
        if (*f == '@' || *f == '=' || *f == '<')
            ++f;
        return (f[0] == c0 || f[0] == c1) && f[1] == 0;
    }
};

struct Mem {                                  // malloc'ed scratch
    void *p = nullptr;
    ~Mem() { free(p); }
    bool get(size_t bytes) { p = malloc(bytes ? bytes : 1); return p != nullptr; }
};

// the 8 characters of a byte, most significant bit first, held in one word so that a key is eight loads
uint64_t g_byte_text[256];

// LSD radix sort of n words (and their weights, if any) on the low `bits` bits; src/dst are swapped per pass, the
// sorted arrays are returned through the references
void radix_sort(uint64_t *&w, uint64_t *&w2, int64_t *&c, int64_t *&c2, size_t n, int bits)
{
    uint32_t hist[1u << MAX_DIGIT];           // (on the stack: a thread_local array costs a TLS lookup per access in a shared object)
    // the fewest passes of at most MAX_DIGIT bits, the bits spread evenly over them: 34 bits are 4 passes of 9, not 3 of 11 and one of 1
    const int passes = (bits + MAX_DIGIT - 1) / MAX_DIGIT;
    const int digit = (bits + passes - 1) / passes;
    for (int sh = 0; sh < bits; sh += digit) {
        const int nb = bits - sh < digit ? bits - sh : digit;
        const size_t nbin = (size_t)1 << nb;
        const uint64_t mask = nbin - 1;
        memset(hist, 0, nbin * sizeof(uint32_t));
        for (size_t i = 0; i < n; ++i)
            ++hist[(w[i] >> sh) & mask];
        if (hist[(w[0] >> sh) & mask] == n)   // every word in one bin: nothing moves
            continue;
        uint32_t run = 0;
        for (size_t k = 0; k < nbin; ++k) {
            const uint32_t h = hist[k];
            hist[k] = run;
            run += h;
        }
        if (c) {
            for (size_t i = 0; i < n; ++i) {
                const size_t d = hist[(w[i] >> sh) & mask]++;
                w2[d] = w[i];
                c2[d] = c[i];
            }
            int64_t *t = c; c = c2; c2 = t;
        } else {
            for (size_t i = 0; i < n; ++i)
                w2[hist[(w[i] >> sh) & mask]++] = w[i];
        }
        uint64_t *t = w; w = w2; w2 = t;
    }
}

// creg_sizes -> the (start, length) slices of the full-width key, last register first; 0 groups: no grouping.
// false: malformed (not mine)
bool read_groups(PyObject *cregs, int num_clbits, int *n_groups, int start[64], int len[64])
{
    *n_groups = 0;
    if (cregs == Py_None)
        return true;
    if (!PyList_CheckExact(cregs) && !PyTuple_CheckExact(cregs))
        return false;
    const Py_ssize_t n = PySequence_Fast_GET_SIZE(cregs);
    if (n <= 1)
        return true;                          // _format_keys groups only from two registers on
    if (n > 64)
        return false;
    int hi = num_clbits;
    for (Py_ssize_t k = n - 1; k >= 0; --k) {
        PyObject *e = PySequence_Fast_GET_ITEM(cregs, k);
        if ((!PyTuple_CheckExact(e) && !PyList_CheckExact(e)) || PySequence_Fast_GET_SIZE(e) != 2)
            return false;
        PyObject *s = PySequence_Fast_GET_ITEM(e, 1);
        if (!PyLong_CheckExact(s))
            return false;
        const long size = PyLong_AsLong(s);
        if (size == -1 && PyErr_Occurred()) {
            PyErr_Clear();
            return false;
        }
        if (size < 1 || size > hi)
            return false;
        start[*n_groups] = num_clbits - hi;
        len[*n_groups] = (int)size;
        ++*n_groups;
        hi -= (int)size;
    }
    return hi == 0;
}

PyObject *counts_dict(PyObject *, PyObject *args)
{
    PyObject *o_words, *o_weights, *o_bits, *o_cregs;
    if (!PyArg_ParseTuple(args, "OOOO", &o_words, &o_weights, &o_bits, &o_cregs)) {
        PyErr_Clear();
        Py_RETURN_NONE;
    }
    if (!PyLong_CheckExact(o_bits))
        Py_RETURN_NONE;
    const long num_clbits = PyLong_AsLong(o_bits);
    if (num_clbits == -1 && PyErr_Occurred()) {
        PyErr_Clear();
        Py_RETURN_NONE;
    }
    if (num_clbits < 0 || num_clbits > 64)
        Py_RETURN_NONE;
    const int w = num_clbits > 0 ? (int)num_clbits : 1;
    int n_groups, g_start[64], g_len[64];
    if (!read_groups(o_cregs, (int)num_clbits, &n_groups, g_start, g_len))
        Py_RETURN_NONE;

    View vw, vc;
    if (!vw.get(o_words, 'Q', 'L'))
        Py_RETURN_NONE;
    const size_t n = (size_t)vw.b.shape[0];
    const bool weighted = o_weights != Py_None;
    if (weighted && (!vc.get(o_weights, 'q', 'l') || (size_t)vc.b.shape[0] != n))
        Py_RETURN_NONE;
    if (n == 0)
        return PyDict_New();
    if (n > 0xffffffffu)                      // the sort counts in 32 bits
        Py_RETURN_NONE;

    // two word arrays (and two weight arrays) for the sort's ping-pong; the caller's buffers are never written
    Mem mw, mc;
    if (!mw.get(2 * n * sizeof(uint64_t)) || (weighted && !mc.get(2 * n * sizeof(int64_t))))
        Py_RETURN_NONE;
    uint64_t *a = static_cast<uint64_t *>(mw.p), *a2 = a + n;
    int64_t *c = weighted ? static_cast<int64_t *>(mc.p) : nullptr, *c2 = weighted ? c + n : nullptr;
    memcpy(a, vw.b.buf, n * sizeof(uint64_t));
    if (weighted)
        memcpy(c, vc.b.buf, n * sizeof(int64_t));
    uint64_t any = 0;
    for (size_t i = 0; i < n; ++i)
        any |= a[i];
    if (w < 64 && (any >> w))                 // a bit the key cannot show: two words could share a key (not mine)
        Py_RETURN_NONE;
    radix_sort(a, a2, c, c2, n, w);

    // A dict sized for n keys up front is never rehashed while it fills: 10-15 % of the call at 4096 distinct words.  The
    // one private call of this module, where the headers still declare it; elsewhere the dict grows as any dict does.
#if PY_VERSION_HEX < 0x030D0000 && !defined(Py_LIMITED_API) && !defined(PYPY_VERSION)
    PyObject *d = _PyDict_NewPresized((Py_ssize_t)n);
#else
    PyObject *d = PyDict_New();
#endif
    if (!d) {
        PyErr_Clear();
        Py_RETURN_NONE;
    }
    const Py_ssize_t keylen = n_groups ? w + n_groups - 1 : w;
    PyObject *one = nullptr;
    for (size_t i = 0; i < n;) {
        const uint64_t v = a[i];
        size_t j = i + 1;
        long long cnt;
        if (weighted) {
            cnt = c[i];
            for (; j < n && a[j] == v; ++j)
                cnt += c[j];
        } else {
            for (; j < n && a[j] == v; ++j) {}
            cnt = (long long)(j - i);
        }
        i = j;
        // the 64 characters of v, most significant bit first; the key is their last w, whole or in register slices
        uint64_t text[8];
        for (int b = 0; b < 8; ++b)
            text[b] = g_byte_text[(v >> (56 - 8 * b)) & 0xff];
        const char *full = reinterpret_cast<const char *>(text) + (64 - w);
        PyObject *key = PyUnicode_New(keylen, 127);
        if (!key)
            goto fail;
        {
            char *out = reinterpret_cast<char *>(PyUnicode_1BYTE_DATA(key));
            if (!n_groups) {
                memcpy(out, full, (size_t)w);
            } else {
                for (int g = 0; g < n_groups; ++g) {
                    if (g)
                        *out++ = ' ';
                    memcpy(out, full + g_start[g], (size_t)g_len[g]);
                    out += g_len[g];
                }
            }
        }
        {
            PyObject *val;
            if (cnt == 1) {
                if (!one && !(one = PyLong_FromLong(1))) {
                    Py_DECREF(key);
                    goto fail;
                }
                val = one;
                Py_INCREF(val);
            } else if (!(val = PyLong_FromLongLong(cnt))) {
                Py_DECREF(key);
                goto fail;
            }
            const int rc = PyDict_SetItem(d, key, val);
            Py_DECREF(key);
            Py_DECREF(val);
            if (rc < 0)
                goto fail;
        }
    }
    Py_XDECREF(one);
    return d;
fail:
    PyErr_Clear();
    Py_XDECREF(one);
    Py_DECREF(d);
    Py_RETURN_NONE;
}

PyMethodDef methods[] = {
    {"counts_dict", counts_dict, METH_VARARGS,
     "counts_dict(words, weights, num_clbits, creg_sizes) -> the dict backend._format_keys builds from np.unique(words) and the "
     "counts (or summed weights), or None (not mine)"},
    {nullptr, nullptr, 0, nullptr}};

PyModuleDef module = {PyModuleDef_HEAD_INIT, "_counts_native", "native counting and key formatting of sampled words (qcmrf_amd.backend)", -1,
                      methods, nullptr, nullptr, nullptr, nullptr};

}  // namespace

PyMODINIT_FUNC PyInit__counts_native(void)
{
    for (int v = 0; v < 256; ++v) {
        char t[8];
        for (int b = 0; b < 8; ++b)
            t[b] = (char)('0' + ((v >> (7 - b)) & 1));
        memcpy(&g_byte_text[v], t, 8);
    }
    return PyModule_Create(&module);
}
