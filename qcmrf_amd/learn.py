"""Parameter learning of the Markov random field behind a QCMRF circuit.

The log-likelihood of data with clique marginals mu-hat under the Gibbs distribution exp(beta <theta, phi(x)> - ln Z) has
the gradient beta (mu-hat - mu(theta)), mu the model's clique marginals: one call of ``QCMRF.marginals`` (all cliques from
one conditioned device pass) or, exactly and on the host, ``mrf.marginals``.
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
