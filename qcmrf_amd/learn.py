"""Parameter learning of the Markov random field behind a QCMRF circuit.

The log-likelihood of data with clique marginals mu-hat under the Gibbs distribution exp(beta <theta, phi(x)> - ln Z) has
the gradient beta (mu-hat - mu(theta)), mu the model's clique marginals: one call of ``QCMRF.marginals`` (all cliques from
one conditioned device pass) or, exactly and on the host, ``mrf.marginals``.  For data rows with missing entries the
gradient of the mean marginal log-likelihood is beta (mean_r mu(theta | observed part of row r) - mu(theta)): one call of
``QCMRF.conditional_marginals`` (all rows from one batched device pass) or ``mrf.conditional_marginals``
(``fit_incomplete``).
"""
from __future__ import annotations

import numpy as np


def gradient(mu_hat, mu, beta=1.0):
    """gradient of the mean log-likelihood with respect to theta: beta (mu-hat - mu)"""
    return beta * (np.asarray(mu_hat, dtype=np.float64) - np.asarray(mu, dtype=np.float64))


def fit(cliques, mu_hat, marginals_fn, theta0=None, steps=100, lr=None, beta=1.0):
    """Plain gradient ascent on the log-likelihood: theta += lr * gradient(mu_hat, marginals_fn(theta)).

    lr defaults to 1 / (beta^2 * number of cliques): the Hessian of the log-partition function is beta^2 Cov(phi), and
    ||phi(x)||^2 = number of cliques for every x (one indicator per clique is 1), so the gradient is Lipschitz with that
    constant and the step never overshoots.  After every step each clique's block is shifted by its maximum
    (theta_C -= max theta_C): the distribution is unchanged and theta <= 0 stays, which the circuit's
    gamma = arccos(exp(beta theta / 2)) / 2 needs.  Returns (theta, [||gradient|| of every step])."""
    sizes = [2 ** len(C) for C in cliques]
    dim = sum(sizes)
    mu_hat = np.asarray(mu_hat, dtype=np.float64)
    if mu_hat.shape != (dim,):
        raise ValueError("mu_hat has shape %r, the model has %d parameters" % (mu_hat.shape, dim))
    theta = np.zeros(dim) if theta0 is None else np.array(theta0, dtype=np.float64)
    if theta.shape != (dim,):
        raise ValueError("theta0 has shape %r, the model has %d parameters" % (theta.shape, dim))
    if lr is None:
        lr = 1.0 / (beta * beta * len(cliques))
    history = []
    for _ in range(int(steps)):
        g = gradient(mu_hat, marginals_fn(theta), beta)
        history.append(float(np.linalg.norm(g)))
        theta = theta + lr * g
        off = 0
        for k in sizes:
            theta[off:off + k] -= theta[off:off + k].max()
            off += k
    return theta, history


def marginals_on(backend, cliques, beta=1.0, **run_options):
    """the ``marginals_fn`` of ``fit`` that prepares the Gibbs state on ``backend``: builds ``QCMRF(cliques, theta)`` and
    returns its ``marginals(backend)``"""
    from .qcmrf import QCMRF

    def marginals_fn(theta):
        qc = QCMRF([list(C) for C in cliques], [float(t) for t in theta], beta=beta)
        return qc.marginals(backend, **run_options)[0]
    return marginals_fn


def fit_incomplete(cliques, rows, conditionals_fn, theta0=None, steps=100, lr=None, beta=1.0):
    """Plain gradient ascent on the mean marginal log-likelihood of data with missing entries: ``rows`` is an int array
    (B, n) with -1 for an unobserved variable, and the gradient is beta (mean_r mu(theta | observed part of row r) -
    mu(theta)).  ``conditionals_fn(theta, rows) -> (mu (B', dimension), p_rows (B',))`` is ``mrf.conditional_marginals``
    on the host or ``conditionals_on(backend, ...)``; mu(theta) comes out of the same call from an all -1 row appended
    to the data.  The same per-clique shift and the same default lr = 1 / (beta^2 * number of cliques) as ``fit``: the
    Hessian is a difference of two covariance matrices of phi, each bounded by that constant's inverse, so the step
    still cannot overshoot.  Returns (theta, history) with history[i] = (mean log p_rows, ||gradient||) at step i."""
    sizes = [2 ** len(C) for C in cliques]
    dim = sum(sizes)
    rows = np.asarray(rows)
    if rows.ndim != 2 or rows.shape[0] == 0:
        raise ValueError("rows is an int array (B, n) with B >= 1")
    theta = np.zeros(dim) if theta0 is None else np.array(theta0, dtype=np.float64)
    if theta.shape != (dim,):
        raise ValueError("theta0 has shape %r, the model has %d parameters" % (theta.shape, dim))
    if lr is None:
        lr = 1.0 / (beta * beta * len(cliques))
    ask = np.concatenate([rows, np.full((1, rows.shape[1]), -1, dtype=rows.dtype)])
    history = []
    for _ in range(int(steps)):
        mu, p_rows = conditionals_fn(theta, ask)
        g = gradient(np.asarray(mu[:-1]).mean(axis=0), mu[-1], beta)
        history.append((float(np.log(p_rows[:-1]).mean()), float(np.linalg.norm(g))))
        theta = theta + lr * g
        off = 0
        for k in sizes:
            theta[off:off + k] -= theta[off:off + k].max()
            off += k
    return theta, history


def conditionals_on(backend, cliques, beta=1.0, **run_options):
    """the ``conditionals_fn`` of ``fit_incomplete`` that prepares the Gibbs state on ``backend``: builds
    ``QCMRF(cliques, theta)`` and returns the first two results of its ``conditional_marginals(backend, rows)``"""
    from .qcmrf import QCMRF

    def conditionals_fn(theta, rows):
        qc = QCMRF([list(C) for C in cliques], [float(t) for t in theta], beta=beta)
        return qc.conditional_marginals(backend, rows, **run_options)[:2]
    return conditionals_fn
