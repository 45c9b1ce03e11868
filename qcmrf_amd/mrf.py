"""Exact (classical) quantities of the Markov random field behind a QCMRF circuit.

The reference's evaluation scripts obtain these from the closed-source ``kiopto_native``
(/root/reference/eval.py:84-93: ``px.backend``, ``px.weights``, ``px.infer(task='partition')``,
``px.logpot``).  For the binary MRFs used there they are elementary: the log-potential of a
joint state x is ``sum_C theta[offset(C) + index(x_C)]`` with the clique state read MSB-first
(the parameter order of /root/reference/QCMRF.py:221,228), so they are computed directly.
"""
from __future__ import annotations

import numpy as np


def num_vertices(cliques):
    return max(v for C in cliques for v in C) + 1


def dimension(cliques):
    """number of parameters = len(px.weights(backend)) of run_experiment.py:26-27"""
    return sum(2 ** len(C) for C in cliques)


def log_potentials(cliques, theta):
    """logpot[xid] for every joint state; xid = int(''.join(x_0 x_1 ... x_{n-1}), 2)
    (the key -> index convention of eval.py:100-101,119)."""
    n = num_vertices(cliques)
    theta = np.asarray(theta, dtype=np.float64)
    if theta.size != dimension(cliques):
        raise ValueError("theta has %d entries, the model has %d parameters" % (theta.size, dimension(cliques)))
    xid = np.arange(2 ** n)
    lp = np.zeros(2 ** n)
    off = 0
    for C in cliques:
        y = np.zeros_like(xid)
        for v in C:
            y = (y << 1) | ((xid >> (n - 1 - v)) & 1)
        lp += theta[off + y]
        off += 2 ** len(C)
    return lp


def gibbs_pmf(cliques, theta, beta=1.0):
    """(p, lnZ): p[xid] = exp(beta*logpot - lnZ)   (eval.py:88-93)"""
    lp = beta * log_potentials(cliques, theta)
    m = lp.max()
    lnZ = m + np.log(np.exp(lp - m).sum())
    return np.exp(lp - lnZ), lnZ


def success_probability(cliques, theta, beta=1.0):
    """probability that every real-part-extraction ancilla reads 0: Z / 2^n"""
    p, lnZ = gibbs_pmf(cliques, theta, beta)
    return float(np.exp(lnZ) / 2 ** num_vertices(cliques))


def clique_index(cliques, x_or_xid):
    """per clique the index of the clique state of every joint state, the first variable of C most significant (the
    order of ``log_potentials``); joint states as xids (1-d) or as an (N, n) array of 0/1"""
    n = num_vertices(cliques)
    a = np.asarray(x_or_xid)
    if a.ndim == 2:
        if a.shape[1] != n:
            raise ValueError("joint states have %d columns, the model has %d variables" % (a.shape[1], n))
        bits = [a[:, v].astype(np.int64) & 1 for v in range(n)]
    elif a.ndim == 1:
        xid = a.astype(np.int64)
        bits = [(xid >> (n - 1 - v)) & 1 for v in range(n)]
    else:
        raise ValueError("joint states are xids (1-d) or an (N, n) array of 0/1")
    out = []
    for C in cliques:
        y = np.zeros(a.shape[0], dtype=np.int64)
        for v in C:
            y = (y << 1) | bits[v]
        out.append(y)
    return out


def marginals(cliques, theta, beta=1.0):
    """mu[offset(C) + y] = P(x_C = y) under the Gibbs distribution, in the order of ``theta``: the exact expectations of
    the sufficient statistics (marginal inference), summed from ``gibbs_pmf``"""
    p, _ = gibbs_pmf(cliques, theta, beta)
    ys = clique_index(cliques, np.arange(p.size))
    return np.concatenate([np.bincount(y, weights=p, minlength=2 ** len(C)) for C, y in zip(cliques, ys)])


def empirical_marginals(cliques, samples):
    """mu-hat: the relative frequency of every clique state in ``samples`` -- an (N, n) array of 0/1, or N xids in the
    ``log_potentials`` convention -- in the order of ``theta``"""
    ys = clique_index(cliques, samples)
    N = np.asarray(samples).shape[0]
    if N == 0:
        raise ValueError("no samples")
    return np.concatenate([np.bincount(y, minlength=2 ** len(C)) / float(N) for C, y in zip(cliques, ys)])


MAP_MAX_K = 64             # QSV_TOP_MAX_K: the most states one device call returns


def _evidence_mask(n, evidence):
    """(mask, value) over xids for ``evidence`` ({variable: 0/1}); a variable outside 0..n-1 is a ValueError"""
    m = val = 0
    for v, b in (evidence or {}).items():
        v = int(v)
        if not 0 <= v < n:
            raise ValueError("evidence variable %d not in 0..%d" % (v, n - 1))
        m |= 1 << (n - 1 - v)
        val |= int(bool(b)) << (n - 1 - v)
    return m, val


def states_of(xid, n):
    """(m, n) int array of the joint states with the given xids: x[i, v] the value of variable v (bit n-1-v of xid)"""
    xid = np.asarray(xid, dtype=np.uint64).astype(np.int64)
    return np.stack([(xid >> (n - 1 - v)) & 1 for v in range(n)], axis=1).astype(np.int64).reshape(xid.size, n)


def map_states(cliques, theta, k=1, beta=1.0, evidence=None):
    """(x, p): the k most probable joint states under the Gibbs distribution given ``evidence`` ({variable: 0/1}) -- exact
    MAP inference (k = 1) and its top-k form, from ``gibbs_pmf``.  ``p`` is renormalised over the states that agree with
    the evidence, descending; equal p by ascending xid (variable v on bit n-1-v, the convention of
    ``hamiltonian_diagonal``).  ``x`` is an int array (m, n), x[i, v] the value of variable v; m = min(k, states that
    agree with the evidence)."""
    n = num_vertices(cliques)
    if int(k) < 1:
        raise ValueError("k = %d, at least 1" % int(k))
    m, val = _evidence_mask(n, evidence)
    p, _ = gibbs_pmf(cliques, theta, beta)
    xid = np.arange(p.size, dtype=np.int64)
    sel = xid[(xid & m) == val]
    ps = p[sel]
    ps = ps / ps.sum()
    order = np.lexsort((sel, -ps))[:int(k)]
    return states_of(sel[order], n), ps[order]


def conditional_marginals(cliques, theta, rows, beta=1.0):
    """(mu, p_rows) for data rows with missing entries: ``rows`` is an int array (B, n) of 0 / 1 and -1 for an unobserved
    variable; ``mu[r]`` holds the clique marginals of the Gibbs distribution given row r's observed values, in the order
    of ``theta`` (an all -1 row gives ``marginals``), and ``p_rows[r]`` is P(observed part of row r).  Exact, summed from
    ``gibbs_pmf``: the host value of ``QCMRF.conditional_marginals``."""
    n = num_vertices(cliques)
    rows = np.asarray(rows)
    if rows.ndim != 2 or rows.shape[1] != n:
        raise ValueError("rows have shape %r, the model has %d variables" % (rows.shape, n))
    if rows.size and not np.isin(rows, (-1, 0, 1)).all():
        raise ValueError("a row entry is 0, 1 or -1 (unobserved)")
    rows = rows.astype(np.int64)
    p, _ = gibbs_pmf(cliques, theta, beta)
    xid = np.arange(p.size)
    ys = clique_index(cliques, xid)
    mu = np.zeros((rows.shape[0], dimension(cliques)))
    p_rows = np.zeros(rows.shape[0])
    for r, row in enumerate(rows):
        w = p.copy()
        for v in range(n):
            if row[v] >= 0:
                w[((xid >> (n - 1 - v)) & 1) != row[v]] = 0.0
        p_rows[r] = w.sum()
        mu[r] = np.concatenate([np.bincount(y, weights=w, minlength=2 ** len(C)) for C, y in zip(cliques, ys)]) / p_rows[r]
    return mu, p_rows
