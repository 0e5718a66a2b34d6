"""The weighted arbiter (tests/pg_info_arbiter.py) pinned on the CPU: with every information matrix the identity it is
tests/pg_arbiter.py, and on a small inconsistent triangle its converged estimate is the minimiser scipy finds for the
stacked residuals L e (Omega = L^T L)."""
import numpy as np
import scipy.optimize

import pg_arbiter
import pg_info_arbiter as arb
from oracle import orc
from pg_fixtures import drifting_loop
from pg_info_fixtures import omega_set


def _edges(est, closures):
    g = orc.PoseGraph()
    for i in range(1, len(est)):
        g.augment_node(est[i])
        for at, to in closures:
            if at == i:
                g.add_loop_closure(to)
    e, X = g.edges(), g.estimates()
    g.close()
    return X, e


def test_identity_information_is_the_unweighted_arbiter():
    gt, est = drifting_loop(40)
    X, edges = _edges(est, [(39, 0)])
    for omegas in (None, [np.eye(6)] * len(edges)):
        Xa, dxa, _ = arb.step(X, edges, omegas)
        Xb, dxb, _ = pg_arbiter.step(X, edges)
        assert np.abs(dxa - dxb).max() <= 1e-15
        assert np.abs(Xa - Xb).max() <= 1e-15


def test_triangle_against_scipy_least_squares():
    """Three vertices, the edges 0 -> 1, 1 -> 2, 2 -> 0 with measurements that do not close (a few centimetres and
    milliradians) and a full information matrix each (set f).  The minimiser of sum |L e|^2 over the local coordinates of
    vertices 1 and 2 (oracle's oplus from the start estimate, oracle's edge error), found by scipy's trust-region
    least squares with three-point differences, against ten Gauss-Newton steps of the arbiter: 1e-9."""
    rng = np.random.default_rng(3)
    X0 = np.array([[0, 0, 0, 0, 0, 0, 1.0],
                   [1.0, 0.1, 0.2, 0, 0.05, 0, 1.0],
                   [0.6, -0.1, 1.1, 0.02, 0.3, -0.01, 1.0]])
    X0[:, 3:] /= np.linalg.norm(X0[:, 3:], axis=1)[:, None]
    pairs = [(0, 1), (1, 2), (2, 0)]
    edges = []
    for (i, j) in pairs:
        e0, _, _ = orc.se3_edge_error(X0[i], X0[j], [0, 0, 0, 0, 0, 0, 1.0])   # = the relative pose's vector form
        z = orc.se3_oplus([0, 0, 0, 0, 0, 0, 1.0], e0 + rng.normal(0, [0.03] * 3 + [0.004] * 3))
        edges.append((i, j, z))
    omegas = omega_set("f", [(i, j, False) for i, j in pairs], seed=9)
    Ls = [np.linalg.cholesky(Om).T for Om in omegas]        # Omega = L^T L

    def estimate(x):
        return np.array([X0[0], orc.se3_oplus(X0[1], x[:6]), orc.se3_oplus(X0[2], x[6:])])

    def residuals(x):
        X = estimate(x)
        return np.concatenate([L @ orc.se3_edge_error(X[i], X[j], z)[0] for L, (i, j, z) in zip(Ls, edges)])

    sol = scipy.optimize.least_squares(residuals, np.zeros(12), method="trf", jac="3-point", xtol=1e-15, ftol=1e-15, gtol=1e-15)
    Xs = estimate(sol.x)
    Xa = arb.optimize(X0, edges, omegas, iters=10)
    assert arb.chi2(Xa, edges, omegas) > 1e-6                 # the triangle does not close: the weights matter
    assert abs(arb.chi2(Xa, edges, omegas) - 2 * sol.cost) <= 1e-12
    dt, dq = arb.deviation(Xa, Xs)
    assert dt <= 1e-9 and dq <= 1e-9, (dt, dq)
    # and the weights do matter: the unweighted minimiser is somewhere else
    Xu = arb.optimize(X0, edges, None, iters=10)
    assert max(arb.deviation(Xu, Xa)) > 1e-4
