"""A blind restatement of the pose graph's robust kernels (include/svo.h, "robust kernels on edges"): rho and the weight w of an edge
at c = chi2 = e^T Omega e, written from the table alone, and the iteratively re-weighted Gauss-Newton step they define -- the weighted
arbiter's step (tests/pg_info_arbiter.py, used as it is) with omegas[k] <- w_k Omega_k.  Nothing here runs the code under test."""
import numpy as np

import pg_info_arbiter as arb

NONE, HUBER, CAUCHY, DCS, GEMAN_MCCLURE = range(5)
KINDS = (HUBER, CAUCHY, DCS, GEMAN_MCCLURE)
NAMES = {NONE: "none", HUBER: "huber", CAUCHY: "cauchy", DCS: "dcs", GEMAN_MCCLURE: "geman-mcclure"}


def rho(kind, delta, c):
    c = np.asarray(c, np.float64)
    if kind == NONE:
        return c.copy()
    if kind == HUBER:
        return np.where(c <= delta * delta, c, 2.0 * delta * np.sqrt(c) - delta * delta)
    if kind == CAUCHY:
        return delta * delta * np.log1p(c / (delta * delta))
    if kind == DCS:
        s = 2.0 * delta / (delta + c)
        return np.where(s >= 1.0, c, s * s * c)
    if kind == GEMAN_MCCLURE:
        return delta * c / (delta + c)
    raise ValueError(kind)


def weight(kind, delta, c):
    c = np.asarray(c, np.float64)
    if kind == NONE:
        return np.ones_like(c)
    if kind == HUBER:
        return np.where(c <= delta * delta, 1.0, delta / np.sqrt(np.maximum(c, 1e-300)))
    if kind == CAUCHY:
        return 1.0 / (1.0 + c / (delta * delta))
    if kind == DCS:
        s = 2.0 * delta / (delta + c)
        return np.where(s >= 1.0, 1.0, s * s)      # g2o's: NOT the derivative of rho = s^2 c
    if kind == GEMAN_MCCLURE:
        return (delta / (delta + c)) ** 2
    raise ValueError(kind)


def edge_chi2(X, edges, omegas=None):
    """chi2 = e^T Omega e per edge at the estimates X, through the oracle's edge function"""
    return np.array([e6 @ arb._om(omegas, k) @ e6 for k, (i, j, e6, A, B) in enumerate(arb.linearize(X, edges))])


def edge_values(X, edges, omegas, kernels):
    """kernels: one (kind, delta) per edge, None = no kernel -> (chi2, w, rho) per edge"""
    c = edge_chi2(X, edges, omegas)
    w, r = np.ones_like(c), c.copy()
    for k, kd in enumerate(kernels):
        if kd is not None and kd[0] != NONE:
            w[k], r[k] = float(weight(kd[0], kd[1], c[k])), float(rho(kd[0], kd[1], c[k]))
    return c, w, r


def weighted_omegas(omegas, w):
    return [w[k] * arb._om(omegas, k) for k in range(len(w))]


def irls_step(X, edges, omegas, kernels):
    """One re-weighted Gauss-Newton step -> (X_next, dx, info of the arbiter, (chi2, w, rho) at X)"""
    c, w, r = edge_values(X, edges, omegas, kernels)
    Xn, dx, info = arb.step(X, edges, weighted_omegas(omegas, w))
    return Xn, dx, info, (c, w, r)


def irls(X, edges, omegas, kernels, iters=10):
    """-> (X after `iters` steps, the list of iterates X_0 ... X_iters)"""
    X = np.array(X, np.float64, copy=True)
    its = [X]
    for _ in range(iters):
        X = irls_step(X, edges, omegas, kernels)[0]
        its.append(X)
    return X, its
