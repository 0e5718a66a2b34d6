"""The arbiter of tests/pg_arbiter.py with per-edge information matrices.

The same scheme with Omega inserted: the edges are linearised by the oracle's orc_se3_edge_error (pg_arbiter.linearize),
H = sum J^T Omega J and b = -sum J^T Omega e are assembled in double, factorised by the same fill-reducing sparse LU, and
the step is refined with 80-bit residuals r = -J^T Omega (e + Ji dxi + Jj dxj), formed edge by edge in longdouble, until
the correction is below 1e-17 |dx|.  The step is applied with the oracle's orc_se3_oplus.  Nothing here runs the code
under test.

Edges are (i, j, Z7) as everywhere; `omegas` is one symmetric 6 x 6 matrix per edge (None = identity), in the coordinates
of the error e = [t ; s q_xyz] (g2o's order)."""
import ctypes as C

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from oracle import orc
from pg_arbiter import deviation, linearize  # noqa: F401  (deviation: re-exported for the tests)

_dp = C.POINTER(C.c_double)
_I6 = np.eye(6)


def _ptr(a):
    return a.ctypes.data_as(_dp)


def _om(omegas, k):
    return _I6 if omegas is None or omegas[k] is None else np.asarray(omegas[k], np.float64)


def normal_equations(lin, omegas, V):
    """H (CSC, 6(V-1) square: vertex 0 is fixed) = sum J^T Omega J and b = -sum J^T Omega e, in double"""
    nb = V - 1
    rows, cols, vals = [], [], []
    b = np.zeros(6 * nb)
    for k, (i, j, e6, A, B) in enumerate(lin):
        Om = _om(omegas, k)
        we = Om @ e6
        for (u, Ju) in ((i, A), (j, B)):
            if u == 0:
                continue
            b[6 * (u - 1):6 * u] -= Ju.T @ we
            for (v, Jv) in ((i, A), (j, B)):
                if v == 0:
                    continue
                r, c = np.meshgrid(np.arange(6 * (u - 1), 6 * u), np.arange(6 * (v - 1), 6 * v), indexing="ij")
                rows.append(r.ravel())
                cols.append(c.ravel())
                vals.append((Ju.T @ (Om @ Jv)).ravel())
    H = sp.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(6 * nb, 6 * nb))
    return H, b


def residual_ld(lin, omegas, V, dx):
    """b - H dx in longdouble, edge by edge: r_u = sum over the edges at u of -J_u^T Omega (e + J_i dx_i + J_j dx_j)"""
    ld = np.longdouble
    r = np.zeros(6 * (V - 1), ld)
    dxl = dx.astype(ld)
    for k, (i, j, e6, A, B) in enumerate(lin):
        v = e6.astype(ld)
        if i:
            v = v + A.astype(ld) @ dxl[6 * (i - 1):6 * i]
        if j:
            v = v + B.astype(ld) @ dxl[6 * (j - 1):6 * j]
        v = _om(omegas, k).astype(ld) @ v
        if i:
            r[6 * (i - 1):6 * i] -= A.T.astype(ld) @ v
        if j:
            r[6 * (j - 1):6 * j] -= B.T.astype(ld) @ v
    return r


def solve_refined(lin, omegas, V, max_steps=6):
    """-> (dx double, info): sparse LU + refinement with longdouble residuals until the correction is below 1e-17 |dx|"""
    H, b = normal_equations(lin, omegas, V)
    lu = spla.splu(H, permc_spec="MMD_AT_PLUS_A", diag_pivot_thresh=0.0, options=dict(SymmetricMode=True))
    dx = lu.solve(b).astype(np.longdouble)
    hist = []
    for _ in range(max_steps):
        r = residual_ld(lin, omegas, V, dx)
        corr = lu.solve(np.asarray(r, np.float64))
        dx = dx + corr.astype(np.longdouble)
        rel = float(np.abs(corr).max() / max(float(np.abs(dx).max()), 1e-300))
        hist.append(rel)
        if rel < 1e-17:
            break
    return np.asarray(dx, np.float64), dict(corrections=hist, residual=float(np.abs(residual_ld(lin, omegas, V, dx)).max()),
                                            H=H, b=b)


def oplus(X, dx):
    """X <- X * fromVectorMQT(dx) for the vertices 1 ... V-1, with the oracle's orc_se3_oplus"""
    lib = orc.load()
    lib.orc_se3_oplus.restype = None
    Xn = np.array(X, np.float64, copy=True)
    out = np.zeros(7)
    for v in range(1, len(X)):
        lib.orc_se3_oplus(_ptr(np.ascontiguousarray(X[v])), _ptr(np.ascontiguousarray(dx[6 * (v - 1):6 * v])), _ptr(out))
        Xn[v] = out
    return Xn


def step(X, edges, omegas=None):
    """One Gauss-Newton step of the weighted graph at the estimates X with the refined solve -> (X_next, dx, info)"""
    lin = linearize(X, edges)
    dx, info = solve_refined(lin, omegas, len(X))
    return oplus(X, dx), dx, info


def plain_cholesky_step(X, info):
    """The yardstick of ONE double-precision solve: the arbiter's own H dx = b by a plain float64 numpy.linalg.cholesky in
    time order (no refinement) -> X_next"""
    L = np.linalg.cholesky(info["H"].toarray())
    dx = sla.solve_triangular(L.T, sla.solve_triangular(L, info["b"], lower=True), lower=False)
    return oplus(X, dx)


def chi2(X, edges, omegas=None):
    return float(sum(e6 @ _om(omegas, k) @ e6 for k, (i, j, e6, A, B) in enumerate(linearize(X, edges))))


def optimize(X, edges, omegas=None, iters=10):
    X = np.array(X, np.float64, copy=True)
    for _ in range(iters):
        X, _, _ = step(X, edges, omegas)
    return X
