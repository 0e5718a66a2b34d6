"""numpy restatement of ros_stereo_slam_amd/csrc/cloud.hip: the indexed cloud's searches by brute force, the normals,
point-to-plane ICP and the information matrix of Open3D's registration module as recalled, operation for operation, so
that the device code can be held to it bit for bit.  Open3D is not available here: every point marked R-<n> is
"upstream, from memory -- verify" (DESIGN.md section 10i lists them); the points marked OURS are this project's choices
where upstream leaves the result open or where we depart from it.

All arithmetic is IEEE float64, one rounding per written operation (no fused multiply-add), evaluated as bracketed.

R-1   registration_icp: pcd = T_init src; result = evaluate; per iteration: update = ComputeTransformation(pcd, target,
      corres); T = update T; pcd = update pcd (incremental, pcd is never recomputed from src); backup = result; result =
      evaluate; stop when |d fitness| < relative_fitness and |d rmse| < relative_rmse.  Defaults 30, 1e-6, 1e-6.
R-2   evaluate: per source point the nearest target point within max_correspondence_distance (SearchHybrid(radius, 1));
      fitness = n_corr / n_src, inlier_rmse = sqrt(sum d2 / n_corr), both 0 without correspondences.
R-3   the radius search is STRICT: a point corresponds iff d2 < max_dist^2.
R-4   TransformationEstimationPointToPlane: r = (s - t) . n_t, J = [s x n_t, n_t] (rotation first), solve J^T J x = -J^T r,
      update = TransformVector6dToMatrix4d(x): rotation Rz(x2) Ry(x1) Rx(x0), translation x[3:6].
R-5   get_information_matrix_from_point_clouds: correspondences of T src at max_dist; Lambda = sum G^T G with the rows of G
      [0, t2, -t1, 1, 0, 0], [-t2, 0, t0, 0, 1, 0], [t1, -t0, 0, 0, 0, 1] at the TARGET point t.
R-6   estimate_normals(KDTreeSearchParamKNN(knn = 30)): the neighbours include the point itself; the normal is the
      eigenvector of the smallest eigenvalue of their covariance; fewer than 3 neighbours, or a zero vector: (0, 0, 1);
      normals are not oriented.

OURS-1  distances: d2 = (dx dx + dy dy) + dz dz in double, dx = p - (double)t; ties go to the lowest target index.
OURS-2  moved points: x' = ((r0 x + r1 y) + r2 z) + t per coordinate; T <- update T by the same bracketing, bottom row fixed.
OURS-3  sums over correspondences: the fixed tree `tree_sum` below (leaf i = source point i, zero without correspondence).
OURS-4  the 6 x 6 solve is a Cholesky factorisation in a fixed order; a pivot <= 0 or a non-finite value gives the IDENTITY
        update, as does an empty correspondence set (upstream: LDLT after a determinant check) -- a stated deviation.
OURS-5  sin / cos of the update are svo_sin / svo_cos of include/svo_math.h (ported in sift_numpy.py).
OURS-6  covariance: the mean m = (sum p) / cnt, then the sum of (p - m)(p - m)^T, both in neighbour order (d2, index), not
        divided (upstream: one pass over cumulants, divided by cnt; eigenvectors do not depend on the scale).
OURS-7  eigenvector: 8 cyclic Jacobi sweeps (0,1), (0,2), (1,2) in double, a rotation skipped when its off-diagonal entry is
        exactly 0; the smallest diagonal entry wins, the lowest index on a tie; normalised by sqrt((x x + y y) + z z).
OURS-8  Lambda is assembled from ten tree sums (t, t t^T's six products, the count), not from per-point 6 x 6 products.
OURS-9  normals are estimated on the target when it has none (upstream would refuse the cloud; the prototype never
        estimates them).
"""
import numpy as np

from sift_numpy import svo_cos, svo_sin

f64 = np.float64
JACOBI_SWEEPS = 8


def new_record():
    """branches reached, for the fixtures' own proof"""
    return dict(ties=0, no_corr=0, identity_update=0, stopped_at=[])


# ---- searches, brute force -------------------------------------------------------------------------------------------
def _d2(p, tgt):
    t = np.asarray(tgt, np.float32).astype(f64)
    dx = p[:, None, 0] - t[None, :, 0]
    dy = p[:, None, 1] - t[None, :, 1]
    dz = p[:, None, 2] - t[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def nearest(p, tgt, max_dist, rec=None):
    """-> (corr [m] int32, d2 [m], 0 where none): OURS-1, R-3"""
    p = np.asarray(p, f64).reshape(-1, 3)
    corr = np.empty(len(p), np.int32)
    dmin = np.empty(len(p))
    for s in range(0, len(p), 256):
        d = _d2(p[s:s + 256], tgt)
        j = np.argmin(d, axis=1)  # the first minimum = the lowest index
        m = d[np.arange(len(j)), j]
        if rec is not None:
            rec["ties"] += int(np.sum((np.sum(d == m[:, None], axis=1) > 1) & (m < max_dist * max_dist)))
        ok = m < max_dist * max_dist
        corr[s:s + 256] = np.where(ok, j, -1)
        dmin[s:s + 256] = np.where(ok, m, 0.0)
    if rec is not None:
        rec["no_corr"] += int(np.sum(corr < 0))
    return corr, dmin


def knn(tgt, k):
    """-> [n, k] int32: the k nearest points of every point by (d2, index), -1 past the end (R-6, OURS-1)"""
    t = np.asarray(tgt, np.float32)
    n = len(t)
    out = np.full((n, k), -1, np.int32)
    for s in range(0, n, 256):
        d = _d2(t[s:s + 256].astype(f64), t)
        o = np.argsort(d, axis=1, kind="stable")[:, :k]
        out[s:s + 256, :o.shape[1]] = o
    return out


# ---- normals ---------------------------------------------------------------------------------------------------------
def _rot(A, V, p, q, r):
    apq = A[:, p, q].copy()
    on = apq != 0.0
    with np.errstate(all="ignore"):
        theta = (A[:, q, q] - A[:, p, p]) / (2.0 * apq)
        t = np.where(theta >= 0.0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
        cs = 1.0 / np.sqrt(t * t + 1.0)
        sn = t * cs
        app = A[:, p, p] - t * apq
        aqq = A[:, q, q] + t * apq
        arp, arq = A[:, r, p].copy(), A[:, r, q].copy()
        nrp = cs * arp - sn * arq
        nrq = sn * arp + cs * arq
    A[:, p, p] = np.where(on, app, A[:, p, p])
    A[:, q, q] = np.where(on, aqq, A[:, q, q])
    A[:, p, q] = A[:, q, p] = np.where(on, 0.0, apq)
    A[:, r, p] = A[:, p, r] = np.where(on, nrp, arp)
    A[:, r, q] = A[:, q, r] = np.where(on, nrq, arq)
    for i in range(3):
        vp, vq = V[:, i, p].copy(), V[:, i, q].copy()
        with np.errstate(all="ignore"):
            V[:, i, p] = np.where(on, cs * vp - sn * vq, vp)
            V[:, i, q] = np.where(on, sn * vp + cs * vq, vq)


def covariance(tgt, nbr):
    """-> (cnt [n], A [n, 3, 3]): OURS-6"""
    t = np.asarray(tgt, np.float32).astype(f64)
    n, k = nbr.shape
    cnt = np.sum(nbr >= 0, axis=1)
    m = np.zeros((n, 3))
    for l in range(k):
        on = nbr[:, l] >= 0
        m = np.where(on[:, None], m + t[np.maximum(nbr[:, l], 0)], m)
    m = m / np.maximum(cnt, 1)[:, None]
    A = np.zeros((n, 3, 3))
    for l in range(k):
        on = nbr[:, l] >= 0
        d = t[np.maximum(nbr[:, l], 0)] - m
        for a in range(3):
            for b in range(a, 3):
                A[:, a, b] = np.where(on, A[:, a, b] + d[:, a] * d[:, b], A[:, a, b])
    for a in range(3):
        for b in range(a):
            A[:, a, b] = A[:, b, a]
    return cnt, A


def normals_from_covariance(cnt, A):
    A = A.copy()
    n = len(A)
    V = np.tile(np.eye(3), (n, 1, 1))
    for _ in range(JACOBI_SWEEPS):
        _rot(A, V, 0, 1, 2)
        _rot(A, V, 0, 2, 1)
        _rot(A, V, 1, 2, 0)
    ev = A[:, 0, 0].copy()
    v = V[:, :, 0].copy()
    for j in (1, 2):
        lt = A[:, j, j] < ev
        ev = np.where(lt, A[:, j, j], ev)
        v = np.where(lt[:, None], V[:, :, j], v)
    nrm = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
    good = (cnt >= 3) & (nrm > 0.0) & (nrm < np.inf)
    with np.errstate(all="ignore"):
        out = v / nrm[:, None]
    out[~good] = (0.0, 0.0, 1.0)
    return out


def normals(tgt, k=30):
    """R-6, OURS-6, OURS-7 -> [n, 3] float64"""
    return normals_from_covariance(*covariance(tgt, knn(tgt, k)))


# ---- the fixed tree (OURS-3) ---------------------------------------------------------------------------------------
def _halve64(x):
    """[g * 64, nv] -> [g, nv]: s[l] += s[l + off], off = 32 .. 1"""
    s = x.reshape(-1, 64, x.shape[1])
    for off in (32, 16, 8, 4, 2, 1):
        s = s[:, :off] + s[:, off:2 * off]
    return s[:, 0]


def _pad64(x):
    n = len(x)
    return np.concatenate([x, np.zeros(((-n) % 64, x.shape[1]))])


def tree_sum(terms):
    """terms [n_src, nv] (zero rows without a correspondence) -> [nv]"""
    C = _halve64(_pad64(_halve64(_pad64(np.asarray(terms, f64)))))
    acc = np.zeros(terms.shape[1])
    for g in range(len(C)):
        acc = acc + C[g]
    return acc


# ---- ICP ---------------------------------------------------------------------------------------------------------------
def move(M, p):
    """OURS-2: M 3x4 (or 4x4), p [n, 3] float64"""
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([((M[i, 0] * x + M[i, 1] * y) + M[i, 2] * z) + M[i, 3] for i in range(3)], axis=1)


def evaluate(pcd, tgt, max_dist, rec=None):
    """R-2 -> (corr, d2, fitness, rmse)"""
    corr, d2 = nearest(pcd, tgt, max_dist, rec)
    s = tree_sum(np.stack([d2, (corr >= 0).astype(f64)], axis=1))
    cnt = s[1]
    return corr, d2, cnt / f64(len(pcd)), (np.sqrt(s[0] / cnt) if cnt > 0 else 0.0)


def icp_terms(pcd, corr, d2, tgt, nrm):
    """[n_src, 29]: 21 J^T J (upper triangle, row-major), 6 J^T r, d2, 1 (R-4)"""
    t = np.asarray(tgt, np.float32).astype(f64)
    on = corr >= 0
    j = np.maximum(corr, 0)
    s, tt, n = pcd, t[j], nrm[j]
    r = ((s[:, 0] - tt[:, 0]) * n[:, 0] + (s[:, 1] - tt[:, 1]) * n[:, 1]) + (s[:, 2] - tt[:, 2]) * n[:, 2]
    J = [s[:, 1] * n[:, 2] - s[:, 2] * n[:, 1], s[:, 2] * n[:, 0] - s[:, 0] * n[:, 2], s[:, 0] * n[:, 1] - s[:, 1] * n[:, 0],
         n[:, 0], n[:, 1], n[:, 2]]
    cols = [J[a] * J[b] for a in range(6) for b in range(a, 6)] + [J[a] * r for a in range(6)] + [d2, np.ones(len(s))]
    return np.where(on[:, None], np.stack(cols, axis=1), 0.0)


def normal_equations(src, tgt, nrm, max_dist, T):
    """one step at T -> (JtJ21, Jtr6, n_corr)"""
    pcd = move(np.asarray(T, f64), np.asarray(src, np.float32).astype(f64))
    corr, d2 = nearest(pcd, tgt, max_dist)
    s = tree_sum(icp_terms(pcd, corr, d2, tgt, nrm))
    return s[:21], s[21:27], int(s[28])


def solve6(A, b):
    """OURS-4 -> x or None"""
    L = np.zeros((6, 6))
    with np.errstate(all="ignore"):
        for j in range(6):
            s = A[j, j]
            for k in range(j):
                s = s - L[j, k] * L[j, k]
            if not (s > 0.0) or not (s < np.inf):
                return None
            L[j, j] = np.sqrt(s)
            for i in range(j + 1, 6):
                u = A[i, j]
                for k in range(j):
                    u = u - L[i, k] * L[j, k]
                L[i, j] = u / L[j, j]
        y = np.zeros(6)
        for i in range(6):
            u = b[i]
            for k in range(i):
                u = u - L[i, k] * y[k]
            y[i] = u / L[i, i]
        x = np.zeros(6)
        for i in range(5, -1, -1):
            u = y[i]
            for k in range(i + 1, 6):
                u = u - L[k, i] * x[k]
            x[i] = u / L[i, i]
    return x if np.all(np.abs(x) < np.inf) else None


def update_matrix(x):
    """R-4, OURS-5 -> 3 x 4"""
    sx, cx, sy, cy, sz, cz = (f64(v) for v in (svo_sin(x[0]), svo_cos(x[0]), svo_sin(x[1]), svo_cos(x[1]), svo_sin(x[2]),
                                              svo_cos(x[2])))
    return np.array([[cz * cy, (cz * sy) * sx - sz * cx, (cz * sy) * cx + sz * sx, x[3]],
                     [sz * cy, (sz * sy) * sx + cz * cx, (sz * sy) * cx - cz * sx, x[4]],
                     [-sy, cy * sx, cy * cx, x[5]]])


def compose(U, T):
    """T <- update T (OURS-2)"""
    out = np.zeros((4, 4))
    out[3, 3] = 1.0
    for i in range(3):
        for j in range(4):
            s = (U[i, 0] * T[0, j] + U[i, 1] * T[1, j]) + U[i, 2] * T[2, j]
            out[i, j] = s + U[i, 3] if j == 3 else s
    return out


def icp(src, tgt, nrm, max_dist, T_init=None, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6, rec=None):
    """R-1 -> (T, fitness, rmse, iterations, corr)"""
    T = np.eye(4) if T_init is None else np.array(T_init, f64).reshape(4, 4)
    T[3] = (0.0, 0.0, 0.0, 1.0)
    pcd = move(T, np.asarray(src, np.float32).astype(f64))
    corr, d2, fit, rmse = evaluate(pcd, tgt, max_dist, rec)
    its = 0
    for it in range(max_iteration):
        s = tree_sum(icp_terms(pcd, corr, d2, tgt, nrm))
        A = np.zeros((6, 6))
        o = 0
        for a in range(6):
            for b in range(a, 6):
                A[a, b] = A[b, a] = s[o]
                o += 1
        x = solve6(A, -s[21:27]) if s[28] > 0 else None
        if x is None:
            if rec is not None:
                rec["identity_update"] += 1
            U = np.eye(4)[:3]
        else:
            U = update_matrix(x)
        T = compose(U, T)
        pcd = move(U, pcd)
        its += 1
        pf, pr = fit, rmse
        corr, d2, fit, rmse = evaluate(pcd, tgt, max_dist, rec)
        if abs(fit - pf) < relative_fitness and abs(rmse - pr) < relative_rmse:
            break
    if rec is not None:
        rec["stopped_at"].append(its)
    return T, fit, rmse, its, corr


def information(src, tgt, max_dist, T):
    """R-5, OURS-8 -> (Lambda [6, 6], n_corr, corr)"""
    pcd = move(np.asarray(T, f64).reshape(4, 4), np.asarray(src, np.float32).astype(f64))
    corr, _ = nearest(pcd, tgt, max_dist)
    t = np.asarray(tgt, np.float32).astype(f64)[np.maximum(corr, 0)]
    cols = [t[:, 0], t[:, 1], t[:, 2], t[:, 0] * t[:, 0], t[:, 1] * t[:, 1], t[:, 2] * t[:, 2], t[:, 0] * t[:, 1],
            t[:, 0] * t[:, 2], t[:, 1] * t[:, 2], np.ones(len(t))]
    a = tree_sum(np.where((corr >= 0)[:, None], np.stack(cols, axis=1), 0.0))
    M = np.zeros((6, 6))
    M[0, 0], M[1, 1], M[2, 2] = a[4] + a[5], a[3] + a[5], a[3] + a[4]
    M[0, 1] = M[1, 0] = -a[6]
    M[0, 2] = M[2, 0] = -a[7]
    M[1, 2] = M[2, 1] = -a[8]
    M[0, 4] = M[4, 0] = -a[2]
    M[0, 5] = M[5, 0] = a[1]
    M[1, 3] = M[3, 1] = a[2]
    M[1, 5] = M[5, 1] = -a[0]
    M[2, 3] = M[3, 2] = -a[1]
    M[2, 4] = M[4, 2] = a[0]
    M[3, 3] = M[4, 4] = M[5, 5] = a[9]
    return M, int(a[9]), corr


def information_einsum(tgt, corr):
    """the same Lambda from the rows of G themselves (the arbiter of OURS-8)"""
    t = np.asarray(tgt, np.float32).astype(f64)[corr[corr >= 0]]
    G = np.zeros((len(t), 3, 6))
    G[:, 0, 1], G[:, 0, 2] = t[:, 2], -t[:, 1]
    G[:, 1, 0], G[:, 1, 2] = -t[:, 2], t[:, 0]
    G[:, 2, 0], G[:, 2, 1] = t[:, 1], -t[:, 0]
    G[:, 0, 3] = G[:, 1, 4] = G[:, 2, 5] = 1.0
    return np.einsum("nra,nrb->ab", G, G)


def pairwise(src, tgt, nrm, dist_coarse=15.0, dist_fine=1.5, rec=None, **kw):
    """pairwiseRegistration -> (T, Lambda, (coarse result), (fine result), n_corr)"""
    c = icp(src, tgt, nrm, dist_coarse, None, rec=rec, **kw)
    f = icp(src, tgt, nrm, dist_fine, c[0], rec=rec, **kw)
    L, n, _ = information(src, tgt, dist_fine, f[0])
    return f[0], L, c, f, n


# ---- from Lambda to an edge ------------------------------------------------------------------------------------------
def skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0.0]])


def edge_information(L, T):
    """Omega = M^-T Lambda M^-1 with M built as stated (the adjoint of T^-1, translation rows first, rotation rows halved)
    and inverted numerically -> 6 x 6"""
    T = np.asarray(T, f64).reshape(4, 4)
    Ri, ti = T[:3, :3].T, -T[:3, :3].T @ T[:3, 3]
    M = np.zeros((6, 6))  # columns: w, v
    M[:3, :3], M[:3, 3:] = skew(ti) @ Ri, Ri
    M[3:, :3] = 0.5 * Ri
    Mi = np.linalg.inv(M)
    return Mi.T @ np.asarray(L, f64).reshape(6, 6) @ Mi
