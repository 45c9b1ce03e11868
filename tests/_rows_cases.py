"""Conditional marginals for a batch of evidence rows (``qsv_marginals_cond_rows``): the row sets the host and the GPU tests
share, the stand-in engine of the host tests, the brute-force host value of ``mrf.conditional_marginals`` and a model of
the post-processing of ``QCMRF.conditional_marginals`` with plantable mistakes.  TEST INFRASTRUCTURE ONLY; written from
the contract in include/qsv.h.

  ROWS_*                  lists of {qubit: 0/1}: the batches of tests/test_gpu_marginals_rows.py
  masks_of                rows -> (masks, vals)
  RowsNumpyEngine         ``MarginalsNumpyEngine`` plus ``marginals_cond_rows``: a loop over its single call, with the entry
                          point's refusals
  all_rows / patterns_of  every row of {-1, 0, 1}^n / the 2^n ways to hide entries of one x
  brute_conditionals      (mu, p_rows) by enumerating the joint states one by one
  modelled_conditionals   the same from per-row unnormalised sums, the way QCMRF.conditional_marginals forms them;
                          ``mistake`` plants one of MISTAKES
"""
from __future__ import annotations

import itertools
import math

import numpy as np

import _marginal_cases as mc
from qcmrf_amd import mrf

MAX_ROWS = 65536
N = mc.N

# ---- the batches of the GPU tests ---------------------------------------------------------------------------------------------
ROWS_MIXED = [mc.FIX_SETS[k] for k in sorted(mc.FIX_SETS)]                # nothing, inner bits, block bits, 11 and all 14 fixed
ROWS_ONE_MASK = [{2: v & 1, 7: (v >> 1) & 1, 13: (v >> 2) & 1} for v in range(8)]
ROWS_19 = [{}, {18: 1, 4: 0}, {q: (q * 3 + 1) % 2 for q in range(2, 14)}, {q: (0b1011001101010110101 >> q) & 1 for q in range(19)}]
GROUPS_19 = mc.GROUP_SETS["pairs"] + [[18, 0, 12, 5, 16, 9, 3, 14]]
ROWS_SHARDS = [{13: 1, 4: 0}, {13: 0}, {12: 1, 13: 1, 0: 1}, {}, {12: 0, 11: 1}]
ROWS_IMPLIED = [{15: 0, 3: 1, 9: 0}, {2: 1, 8: 0}, {13: 1, 14: 0}, {}, {15: 1}]      # the last one: the zero half


def masks_of(rows):
    mv = [mc.mask_of(f) for f in rows]
    return [m for m, _ in mv], [v for _, v in mv]


def nbins(groups):
    return sum(1 << len(g) for g in groups)


def single_flat(eng, groups, fixed):
    """the single call's answer as the batched call lays it out: the groups' bins one after the other, and the mass"""
    parts, mass = eng.marginals_cond(groups, *mc.mask_of(fixed))
    return np.concatenate([np.asarray(p, dtype=np.float64) for p in parts] or [np.zeros(0)]), mass


# ---- the stand-in engine ------------------------------------------------------------------------------------------------------
class RowsNumpyEngine(mc.MarginalsNumpyEngine):
    """MarginalsNumpyEngine with ``marginals_cond_rows``: the single call row by row (that is the contract)"""

    def marginals_cond_rows(self, groups, masks, vals):
        B = len(masks)
        if len(vals) != B:
            raise ValueError("%d masks but %d values" % (B, len(vals)))
        if not 1 <= B <= MAX_ROWS:
            raise ValueError("%d rows, 1..%d supported" % (B, MAX_ROWS))
        for r, (m, v) in enumerate(zip(masks, vals)):
            if v & ~m:
                raise ValueError("row %d: fix_val has bits outside fix_mask" % r)
            if m >> self.n_qubits:
                raise ValueError("row %d: fix_mask has bits at or above qubit %d" % (r, self.n_qubits))
        out = np.zeros((B, max(1, nbins(groups))), dtype=np.float64)
        mass = np.zeros(B, dtype=np.float64)
        calls = getattr(self, "marginal_calls", 0)
        for r in range(B):
            parts, mass[r] = self.marginals_cond(groups, int(masks[r]), int(vals[r]))
            out[r, :nbins(groups)] = np.concatenate(parts)
        self.marginal_calls = calls                                          # the loop stands for ONE batched call
        self.rows_calls = getattr(self, "rows_calls", 0) + 1
        return out, mass


def factory(n, devices=(0,), rank=None, world_size=None):
    return RowsNumpyEngine(n, len(devices))


# ---- rows of a model ----------------------------------------------------------------------------------------------------------
GRAPHS = {"chain4": [[0, 1], [1, 2], [2, 3]], "triangles": [[0, 1, 2], [2, 3, 4]], "k4": [[0, 1, 2, 3]]}


def all_rows(n):
    return np.array(list(itertools.product((-1, 0, 1), repeat=n)), dtype=np.int64)


def patterns_of(x):
    """the 2^n rows that hide a subset of x's entries: all hidden first, fully observed last"""
    x = np.asarray(x, dtype=np.int64)
    return np.array([[x[v] if (m >> v) & 1 else -1 for v in range(x.size)] for m in range(1 << x.size)], dtype=np.int64)


def sampled_rows(cliques, theta, B, hidden=0.3, seed=0, beta=1.0):
    """B joint states drawn from the Gibbs distribution, every entry hidden with probability ``hidden``"""
    n = mrf.num_vertices(cliques)
    p, _ = mrf.gibbs_pmf(cliques, theta, beta)
    rs = np.random.RandomState(seed)
    xid = rs.choice(p.size, size=B, p=p / p.sum())
    rows = np.array([[(x >> (n - 1 - v)) & 1 for v in range(n)] for x in xid], dtype=np.int64)
    rows[rs.random_sample(rows.shape) < hidden] = -1
    return rows


def brute_conditionals(cliques, theta, rows, beta=1.0):
    n = mrf.num_vertices(cliques)
    p, _ = mrf.gibbs_pmf(cliques, theta, beta)
    mu = np.zeros((len(rows), mrf.dimension(cliques)))
    p_rows = np.zeros(len(rows))
    for r, row in enumerate(rows):
        acc = [[] for _ in range(mrf.dimension(cliques))]
        tot = []
        for xid in range(1 << n):
            x = [(xid >> (n - 1 - v)) & 1 for v in range(n)]
            if any(row[v] >= 0 and row[v] != x[v] for v in range(n)):
                continue
            tot.append(p[xid])
            off = 0
            for C in cliques:
                y = int("".join(str(x[v]) for v in C), 2)
                acc[off + y].append(p[xid])
                off += 2 ** len(C)
        p_rows[r] = math.fsum(tot)
        mu[r] = [math.fsum(a) / p_rows[r] for a in acc]
    return mu, p_rows


MISTAKES = ["row_value_ignored", "masses_swapped", "denominator_from_wrong_row", "bin_order_reversed"]


def modelled_conditionals(cliques, theta, rows, beta=1.0, mistake=None):
    """(mu, p_rows) from unnormalised per-row sums over the variables' qubits (variable v on qubit n-1-v, bin bit b <->
    group[b], the extra last row unconditioned) -- the shape of the device result -- normalised as
    ``QCMRF.conditional_marginals`` normalises it"""
    n = mrf.num_vertices(cliques)
    w = 0.37 * mrf.gibbs_pmf(cliques, theta, beta)[0]                      # not normalised: the device's sums are not either
    p = np.zeros(1 << n)
    xid = np.arange(1 << n)
    p[xid] = w                                                               # index = sum x_v << (n-1-v): the xid itself
    groups = [[n - 1 - v for v in reversed(C)] for C in cliques]
    if mistake == "bin_order_reversed":
        groups = [[n - 1 - v for v in C] for C in cliques]
    fixed_rows = [{n - 1 - v: int(row[v]) for v in range(n) if row[v] >= 0} for row in rows] + [{}]
    if mistake == "row_value_ignored":
        fixed_rows = [{q: 0 for q in f} for f in fixed_rows]
    out, mass = [], []
    for f in fixed_rows:
        parts, m = mc.marginals_reference(p, groups, *mc.mask_of(f))
        out.append(np.concatenate(parts))
        mass.append(m)
    out, mass = np.array(out), np.array(mass)
    B = len(rows)
    own = mass[:B].copy()
    if mistake == "masses_swapped":
        own = own[::-1].copy()
    den = mass[0] if mistake == "denominator_from_wrong_row" else mass[-1]
    return out[:B] / own[:, None], own / den
