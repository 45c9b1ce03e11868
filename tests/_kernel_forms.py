"""Helpers of tests/test_gpu_kernel_forms.py: a gate sequence as plain data, applied to an Engine and to the numpy oracle.

A gate is a tuple whose first entry names the entry point:
    ("u", t, m, ctrls, vals)      apply_1q            ("x", ctrls, t, vals)      apply_mcx
    ("ph", qubits, angle, vals)   apply_mcphase       ("diag", qubits, table)    apply_diag
    ("mux", selects, t, mats)     apply_mux           ("kq", qubits, u)          apply_kq
    ("swap", a, b)                swap_layout of one pair
so that one sequence can run on several engines (options, grid sizes, shard counts) and once on the host."""
import numpy as np

from oracle import sv_numpy as sv


def rand_state(n, seed):
    rs = np.random.RandomState(seed)
    v = rs.randn(2 ** n) + 1j * rs.randn(2 ** n)
    return v / np.linalg.norm(v)


def rand_u(k, seed):
    rs = np.random.RandomState(seed)
    a = rs.randn(2 ** k, 2 ** k) + 1j * rs.randn(2 ** k, 2 ** k)
    q, _ = np.linalg.qr(a)
    return q


def rand_table(k, seed):
    return np.exp(1j * np.random.RandomState(seed).uniform(-3, 3, size=2 ** k))


def rand_mats(k, seed):
    return np.array([rand_u(1, seed + j) for j in range(2 ** k)])


def swap_bits_index(n, a, b):
    """i with bits a and b exchanged, for every i < 2^n"""
    i = np.arange(2 ** n, dtype=np.int64)
    d = ((i >> a) ^ (i >> b)) & 1
    return i ^ (d << a) ^ (d << b)


def apply_engine(e, g):
    kind = g[0]
    if kind == "u":
        e.apply_1q(g[1], g[2], g[3], g[4])
    elif kind == "x":
        e.apply_mcx(g[1], g[2], g[3])
    elif kind == "ph":
        e.apply_mcphase(g[1], g[2], g[3])
    elif kind == "diag":
        e.apply_diag(g[1], g[2])
    elif kind == "mux":
        e.apply_mux(g[1], g[2], g[3])
    elif kind == "kq":
        e.apply_kq(g[1], g[2])
    elif kind == "swap":
        e.swap_layout([g[1]], [g[2]])
    else:
        raise ValueError("unknown gate %r" % (kind,))


def apply_numpy(ref, g):
    """the same gate on the host vector (returns it: a swap makes a new array)"""
    kind = g[0]
    if kind == "u":
        sv.apply_1q(ref, g[1], g[2], g[3], g[4])
    elif kind == "x":
        sv.apply_mcx(ref, g[1], g[2], g[3])
    elif kind == "ph":
        sv.apply_mcphase(ref, g[1], g[2], g[3])
    elif kind == "diag":
        sv.apply_diag(ref, g[1], g[2])
    elif kind == "mux":
        sv.apply_mux(ref, g[1], g[2], g[3])
    elif kind == "kq":
        sv.apply_kq(ref, g[1], g[2])
    elif kind == "swap":
        ref = ref[swap_bits_index(sv.nqubits(ref), g[1], g[2])]
    else:
        raise ValueError("unknown gate %r" % (kind,))
    return ref


def run_engine(lib, n, state, gates, options=(), devices=(0,)):
    """the amplitudes ``gates`` leave on an engine of ``n`` qubits started from ``state``; options: (name, value) pairs"""
    with lib.Engine(n, devices=devices) as e:
        for name, value in options:
            e.set_option(name, value)
        e.set_amplitudes(0, state)
        for g in gates:
            apply_engine(e, g)
        return e.amplitudes()


def run_numpy(state, gates):
    ref = state.copy()
    for g in gates:
        ref = apply_numpy(ref, g)
    return ref


_LAST = {}


def reference(key, n, seed, make_gates):
    """(state, gates, reference) of a case, computed once: the cases of one parametrised test run one after the other and
    share it (one entry is kept, 2^22 amplitudes are 64 MiB); nobody writes to the three"""
    if key not in _LAST:
        _LAST.clear()
        state = rand_state(n, seed)
        gates = make_gates()
        ref = run_numpy(state, gates)
        for a in (state, ref):
            a.setflags(write=False)
        _LAST[key] = (state, gates, ref)
    return _LAST[key]


def marginal(p, qubits, fix_mask=0, fix_val=0):
    """sum of p over the indices g with (g & fix_mask) == fix_val, binned by the bits ``qubits`` of g (bit b <- qubits[b])"""
    idx = np.arange(p.size, dtype=np.int64)
    j = np.zeros_like(idx)
    for b, q in enumerate(qubits):
        j |= ((idx >> q) & 1) << b
    sel = (idx & fix_mask) == fix_val
    return np.bincount(j[sel], weights=p[sel], minlength=1 << len(qubits))
