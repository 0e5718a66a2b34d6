"""float64 numpy restatement of svo_ba_window (include/svo.h): g2o's OptimizationAlgorithmLevenberg over BlockSolver<6,3> with several
VertexSE3Expmap (some held), free marginalised points, EdgeSE3ProjectXYZ / EdgeStereoSE3ProjectXYZ observations stored CSR by point,
RobustKernelHuber as robustify applies it.  Schur form, analytic Jacobians; written from the issue's text and g2o's formulas, not
from csrc/ba_window.hip.  tests/test_ba_window_numpy.py holds it to a dense LM with numeric Jacobians and to the standing oracle."""
import numpy as np

from ba_fixtures import se3_exp

DEFAULTS = dict(fx=718.856, fy=718.856, cx=607.1928, cy=185.2157, bf=718.856 * 0.54, iterations=10, huber_mono=0.0, huber_stereo=0.0)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def huber(e2, delta):
    """RobustKernelHuber::robustify -> (rho, rho')."""
    e2 = np.asarray(e2, np.float64)
    delta = np.broadcast_to(np.asarray(delta, np.float64), e2.shape)
    out = (delta > 0) & (e2 > delta * delta)
    s = np.sqrt(np.where(out, e2, 1.0))
    return np.where(out, 2 * s * delta - delta * delta, e2), np.where(out, delta / s, 1.0)


def residuals(P, X, obs_point, obs_pose, obs_uvr, prm):
    """(n_obs, 3) residuals (third 0 for mono), the stereo mask and the camera-frame points."""
    R, t = P[obs_pose, :9].reshape(-1, 3, 3), P[obs_pose, 9:]
    xc = np.einsum("nij,nj->ni", R, X[obs_point]) + t
    x, y, z = xc.T
    z_ = obs_uvr.astype(np.float64)
    stereo = ~np.isnan(z_[:, 2])
    e = np.zeros((len(obs_pose), 3))
    e[:, 0] = z_[:, 0] - (x / z * prm["fx"] + prm["cx"])
    e[:, 1] = z_[:, 1] - (y / z * prm["fy"] + prm["cy"])
    e[stereo, 2] = z_[stereo, 2] - (x[stereo] / z[stereo] * prm["fx"] + prm["cx"] - prm["bf"] / z[stereo])
    return e, stereo, xc


def robust(e, stereo, prm, no_kernel=False):
    e2 = (e * e).sum(1)
    if no_kernel:
        return e2, None
    return huber(e2, np.where(stereo, prm["huber_stereo"], prm["huber_mono"]))


def linearize(P, X, obs_point, obs_pose, obs_uvr, prm):
    """e, A = de/dpoint (n, 3, 3), B = de/dpose (n, 3, 6; [omega; upsilon]), stereo mask."""
    e, stereo, xc = residuals(P, X, obs_point, obs_pose, obs_uvr, prm)
    R = P[obs_pose, :9].reshape(-1, 3, 3)
    x, y, z = xc.T
    fx, fy, bf = prm["fx"], prm["fy"], prm["bf"]
    z2 = z * z
    n = len(z)
    A = np.zeros((n, 3, 3))
    A[:, 0, :] = -fx * R[:, 0, :] / z[:, None] + fx * (x / z2)[:, None] * R[:, 2, :]
    A[:, 1, :] = -fy * R[:, 1, :] / z[:, None] + fy * (y / z2)[:, None] * R[:, 2, :]
    A[:, 2, :] = A[:, 0, :] - (bf / z2)[:, None] * R[:, 2, :]
    B = np.zeros((n, 3, 6))
    B[:, 0, 0] = x * y / z2 * fx
    B[:, 0, 1] = -(1 + x * x / z2) * fx
    B[:, 0, 2] = y / z * fx
    B[:, 0, 3] = -1 / z * fx
    B[:, 0, 5] = x / z2 * fx
    B[:, 1, 0] = (1 + y * y / z2) * fy
    B[:, 1, 1] = -x * y / z2 * fy
    B[:, 1, 2] = -x / z * fy
    B[:, 1, 4] = -1 / z * fy
    B[:, 1, 5] = y / z2 * fy
    B[:, 2, :] = B[:, 0, :]
    B[:, 2, 0] -= bf * y / z2
    B[:, 2, 1] += bf * x / z2
    B[:, 2, 5] -= bf / z2
    A[~stereo, 2, :] = 0
    B[~stereo, 2, :] = 0
    return e, A, B, stereo


def csr_points(obs_start):
    obs_start = np.asarray(obs_start, np.int64)
    return np.repeat(np.arange(len(obs_start) - 1), np.diff(obs_start))


def free_numbering(fixed):
    fixed = np.asarray(fixed).astype(bool)
    idx = np.full(len(fixed), -1)
    idx[~fixed] = np.arange((~fixed).sum())
    return idx, np.flatnonzero(~fixed)


def ba_window(poses, fixed, pts3d, obs_start, obs_pose, obs_uvr, prm=None, no_kernel=False, trace=None):
    """-> (poses (P, 12), points (N, 3), per-observation e^T e, info).  `trace`: a list that receives (accepted, rho) per trial."""
    prm = params() if prm is None else prm
    P = np.array(poses, np.float64).reshape(-1, 12).copy()
    X = np.asarray(pts3d, np.float32).reshape(-1, 3).astype(np.float64)
    obs_pose = np.asarray(obs_pose, np.int64)
    obs_uvr = np.asarray(obs_uvr, np.float32).reshape(-1, 3)
    op = csr_points(obs_start)
    N = len(X)
    fidx, flist = free_numbering(fixed)
    D = 6 * len(flist)
    of = fidx[obs_pose]
    fo = np.flatnonzero(of >= 0)   # observations by free poses
    rows = (6 * of[fo])[:, None] + np.arange(6)[None, :]

    def chi_of(P, X):
        e, stereo, _ = residuals(P, X, op, obs_pose, obs_uvr, prm)
        return robust(e, stereo, prm, no_kernel)[0].sum()

    chi = chi_of(P, X)
    chi_first = chi_last = chi
    lam, ni, trials, it_run = 0.0, 2.0, 0, 0
    for it in range(prm["iterations"]):
        chi = chi_of(P, X)
        e, A, B, stereo = linearize(P, X, op, obs_pose, obs_uvr, prm)
        w = robust(e, stereo, prm, no_kernel)[1]
        wA, we = (A, e) if w is None else (A * w[:, None, None], e * w[:, None])
        Hll, bl = np.zeros((N, 3, 3)), np.zeros((N, 3))
        np.add.at(Hll, op, np.einsum("nri,nrj->nij", A, wA))
        np.add.at(bl, op, -np.einsum("nri,nr->ni", A, we))
        Hpl = np.einsum("nri,nrj->nij", B, wA)   # (n_obs, 6, 3)
        Hpp, bp = np.zeros((D, D)), np.zeros(D)
        for o in fo:   # block diagonal
            f = of[o]
            Hpp[6 * f:6 * f + 6, 6 * f:6 * f + 6] += B[o].T @ (B[o] if w is None else w[o] * B[o])
            bp[6 * f:6 * f + 6] += -B[o].T @ we[o]
        W = np.zeros((N, D, 3))
        W[op[fo][:, None], rows, :] = Hpl[fo]
        if it == 0:
            lam = 1e-5 * max(np.abs(np.diag(Hpp)).max(), np.abs(Hll[:, [0, 1, 2], [0, 1, 2]]).max())
            ni = 2.0
        rho, qmax, bad = 0.0, 0, False
        while True:
            Vi = np.linalg.inv(Hll + lam * np.eye(3))
            S = Hpp + lam * np.eye(D) - np.einsum("ndk,nkl,nel->de", W, Vi, W)
            bs = bp - np.einsum("ndk,nkl,nl->d", W, Vi, bl)
            solved = True
            try:
                L = np.linalg.cholesky(S)
                dp = np.linalg.solve(L.T, np.linalg.solve(L, bs))
            except np.linalg.LinAlgError:
                solved = False
            temp, scale = np.finfo(np.float64).max, 0.0
            if solved:
                dl = np.einsum("nkl,nl->nk", Vi, bl - np.einsum("ndk,d->nk", W, dp))
                Pn = P.copy()
                for f, j in enumerate(flist):
                    E, u = se3_exp(dp[6 * f:6 * f + 6])
                    Pn[j, :9] = (E @ P[j, :9].reshape(3, 3)).ravel()
                    Pn[j, 9:] = E @ P[j, 9:] + u
                Xn = X + dl
                temp = chi_of(Pn, Xn)
                scale = (dl * (lam * dl + bl)).sum() + dp @ (lam * dp + bp)
            trials += 1
            rho = (chi - temp) / (scale + 1e-3)
            ok = bool(rho > 0 and np.isfinite(temp) and solved)
            if trace is not None:
                trace.append((ok, rho))
            if ok:
                lam *= max(1 / 3, min(2 / 3, 1 - (2 * rho - 1) ** 3))
                ni = 2.0
                P, X = Pn, Xn
                chi_last = temp
            else:
                lam *= ni
                ni *= 2
                if not np.isfinite(lam):
                    bad = True
                    break
            qmax += 1
            if not (rho < 0 and qmax < 10):
                break
        it_run = it + 1
        if qmax == 10 or rho == 0 or bad:
            break
    e, _, _ = residuals(P, X, op, obs_pose, obs_uvr, prm)
    info = dict(chi2_before=chi_first, chi2_after=chi_last, lambda_final=lam, iterations=it_run, trials=trials,
                observations=len(obs_pose))
    return P, X, (e * e).sum(1), info
