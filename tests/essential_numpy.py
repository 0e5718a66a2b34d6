"""numpy restatement of findEssentialMat (RANSAC) and recoverPose as ros_stereo_slam_amd/csrc/essential.hip states them.

OpenCV 3.2's recipe (five-point.cpp, ptsetreg.cpp), with the implementer's choices where OpenCV uses its own SVD and
solvePoly, restated independently of the HIP file:
  * K-normalisation ((x - cx) / fx, (y - cy) / fy) in double; threshold / ((fx + fy) / 2).
  * the 5 x 9 system [x2 x1, x2 y1, x2, y2 x1, y2 y1, y2, x1, y1, 1]; null space by Gauss-Jordan with full pivoting
    (the first entry, row-major, of the largest magnitude), the four vectors orthonormalised by modified Gram-Schmidt;
  * the ten cubic constraints derived here by products of polynomials (a dict per polynomial, not a pasted table), in
    OpenCV's monomial order; A[:, :10]^-1 A[:, 10:]; B (3 x 13) as runKernel builds it; det B(z) by polynomial products;
  * roots by np.roots with OpenCV's |imag| <= 1e-10 filter, in ascending order; (x, y) from the null vector of B(z)
    (SVD), dropped when its third component is below 1e-10; four Gauss-Newton steps on the ten constraints in
    (x, y, z); E at unit norm, its largest entry positive; dropped when a constraint residual exceeds 1e-6;
  * the Sampson error in double stored as float, inliers err <= (float) thr^2;
  * the sequential RANSAC loop with samples from the oracle's orc_draw_subset_plain and the bound from
    orc_update_num_iters (ctypes); first-best-wins over count > max(best, 4);
  * decomposeEssentialMat with the HIP file's sign rule, the DLT per pair (numpy SVD) and the cheirality test.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

# OpenCV's monomial order (exponents of x, y, z): getCoeffMat's columns
MONO = [(3, 0, 0), (0, 3, 0), (2, 1, 0), (1, 2, 0), (2, 0, 1), (2, 0, 0), (0, 2, 1), (0, 2, 0), (1, 1, 1), (1, 1, 0),
        (1, 0, 2), (1, 0, 1), (1, 0, 0), (0, 1, 2), (0, 1, 1), (0, 1, 0), (0, 0, 3), (0, 0, 2), (0, 0, 1), (0, 0, 0)]
W = np.array([[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])


def _lib():
    from oracle import orc

    return orc.load()


def draw(n, seed, it):
    """the 5-sample of iteration `it` -> (ok, indices) (the oracle's orc_draw_subset_plain)."""
    idx = np.zeros(5, np.int32)
    f = _lib().orc_draw_subset_plain
    f.argtypes = [C.c_uint64, C.c_uint32, C.c_int, C.c_int, C.c_void_p]
    f.restype = C.c_int
    ok = f(seed, it, n, 5, C.c_void_p(idx.ctypes.data))
    return bool(ok), idx


def update_num_iters(p, ep, model_points, max_iters):
    f = _lib().orc_update_num_iters
    f.argtypes = [C.c_double, C.c_double, C.c_int, C.c_int]
    f.restype = C.c_int
    return f(p, ep, model_points, max_iters)


def normalise(p, K4):
    fx, fy, cx, cy = (float(v) for v in K4)
    p = np.asarray(p, np.float32).reshape(-1, 2).astype(np.float64)
    return np.stack([(p[:, 0] - cx) / fx, (p[:, 1] - cy) / fy], 1)


# ---- polynomials as {(a, b, c): coefficient} ----
def pmul(p, q):
    out = {}
    for ka, va in p.items():
        for kb, vb in q.items():
            k = (ka[0] + kb[0], ka[1] + kb[1], ka[2] + kb[2])
            out[k] = out.get(k, 0.0) + va * vb
    return out


def padd(*terms):
    out = {}
    for s, p in terms:
        for k, v in p.items():
            out[k] = out.get(k, 0.0) + s * v
    return out


def null_basis(q1, q2):
    """the four orthonormalised null vectors of the 5 x 9 system (rows of a 4 x 9 array), None when degenerate."""
    x1, y1, x2, y2 = q1[:, 0], q1[:, 1], q2[:, 0], q2[:, 1]
    A = np.stack([x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, np.ones(5)], 1)
    perm = np.arange(9)
    for k in range(5):
        sub = np.abs(A[k:, k:])
        if not sub.max() >= 1e-12:
            return None
        r, c = np.unravel_index(int(np.argmax(sub)), sub.shape)
        r, c = r + k, c + k
        A[[k, r]] = A[[r, k]]
        A[:, [k, c]] = A[:, [c, k]]
        perm[[k, c]] = perm[[c, k]]
        A[k] = A[k] / A[k, k]
        for i in range(5):
            if i != k:
                A[i] = A[i] - A[i, k] * A[k]
    basis = np.zeros((4, 9))
    for f in range(4):
        e = np.zeros(9)
        e[perm[:5]] = -A[:, 5 + f]
        e[perm[5 + f]] = 1.0
        for g in range(f):
            e = e - (basis[g] @ e) * basis[g]
        basis[f] = e / np.linalg.norm(e)
    return basis


def coeff_matrix(basis):
    """the 10 x 20 matrix of det(E) = 0 and 2 E E^T E - tr(E E^T) E = 0, E = x E0 + y E1 + z E2 + E3."""
    L = [{(1, 0, 0): basis[0, m], (0, 1, 0): basis[1, m], (0, 0, 1): basis[2, m], (0, 0, 0): basis[3, m]}
         for m in range(9)]
    E = [[L[3 * i + j] for j in range(3)] for i in range(3)]
    EEt = [[padd(*[(1.0, pmul(E[i][k], E[j][k])) for k in range(3)]) for j in range(3)] for i in range(3)]
    tr = padd((1.0, EEt[0][0]), (1.0, EEt[1][1]), (1.0, EEt[2][2]))
    rows = []
    for i in range(3):
        for j in range(3):
            rows.append(padd(*[(2.0, pmul(EEt[i][k], E[k][j])) for k in range(3)], (-1.0, pmul(tr, E[i][j]))))
    minor = lambda a, b, c, d: padd((1.0, pmul(a, d)), (-1.0, pmul(b, c)))  # noqa: E731
    det = padd((1.0, pmul(E[0][0], minor(E[1][1], E[1][2], E[2][1], E[2][2]))),
               (-1.0, pmul(E[0][1], minor(E[1][0], E[1][2], E[2][0], E[2][2]))),
               (1.0, pmul(E[0][2], minor(E[1][0], E[1][1], E[2][0], E[2][1]))))
    rows.append(det)
    return np.array([[r.get(m, 0.0) for m in MONO] for r in rows])


def b_matrix(A):
    Cm = np.linalg.solve(A[:, :10], A[:, 10:])
    B = np.zeros((3, 13))
    for i in range(3):
        a1, a2 = Cm[2 * i + 4], Cm[2 * i + 5]
        r1, r2 = np.zeros(13), np.zeros(13)
        r1[1:4], r1[5:8], r1[9:13] = a1[0:3], a1[3:6], a1[6:10]
        r2[0:3], r2[4:7], r2[8:12] = a2[0:3], a2[3:6], a2[6:10]
        B[i] = r1 - r2
    return B


def det_poly(B):
    """det B(z), coefficients in ascending powers (degree 10)."""
    P = np.polynomial.polynomial
    b = [[B[j, 3::-1], B[j, 7:3:-1], B[j, 12:7:-1]] for j in range(3)]  # ascending
    m0 = P.polysub(P.polymul(b[1][1], b[2][2]), P.polymul(b[1][2], b[2][1]))
    m1 = P.polysub(P.polymul(b[1][0], b[2][2]), P.polymul(b[1][2], b[2][0]))
    m2 = P.polysub(P.polymul(b[1][0], b[2][1]), P.polymul(b[1][1], b[2][0]))
    p = P.polyadd(P.polysub(P.polymul(b[0][0], m0), P.polymul(b[0][1], m1)), P.polymul(b[0][2], m2))
    out = np.zeros(11)
    out[:len(p)] = p
    return out


def sign_fix(E):
    E = E / np.linalg.norm(E)
    f = E.ravel()
    im = int(np.argmax(np.abs(f)))
    return E if f[im] >= 0 else -E


def five_point(q1, q2):
    """solutions (k x 3 x 3) of the five-point problem on normalised coordinates, ascending z."""
    q1, q2 = np.asarray(q1, np.float64).reshape(5, 2), np.asarray(q2, np.float64).reshape(5, 2)
    basis = null_basis(q1, q2)
    if basis is None:
        return np.zeros((0, 3, 3))
    A = coeff_matrix(basis)
    B = b_matrix(A)
    p = det_poly(B)
    nz = np.nonzero(p)[0]
    if len(nz) == 0 or nz[-1] == 0:
        return np.zeros((0, 3, 3))
    roots = np.roots(p[:nz[-1] + 1][::-1])
    zs = np.sort(roots[np.abs(roots.imag) <= 1e-10].real)
    sols = []
    for z in zs:
        Bz = np.stack([B[:, 0] * z ** 3 + B[:, 1] * z ** 2 + B[:, 2] * z + B[:, 3],
                       B[:, 4] * z ** 3 + B[:, 5] * z ** 2 + B[:, 6] * z + B[:, 7],
                       B[:, 8] * z ** 4 + B[:, 9] * z ** 3 + B[:, 10] * z ** 2 + B[:, 11] * z + B[:, 12]], 1)
        v = np.linalg.svd(Bz)[2][-1]
        if abs(v[2]) < 1e-10:
            continue
        xyz = polish(A, np.array([v[0] / v[2], v[1] / v[2], z]))
        E = sign_fix((basis[0] * xyz[0] + basis[1] * xyz[1] + basis[2] * xyz[2] + basis[3]).reshape(3, 3))
        if max(constraint_residuals(E)) <= 1e-6:
            sols.append(E)
    return np.array(sols).reshape(-1, 3, 3)


def polish(A, xyz, steps=4):
    """Gauss-Newton on the ten cubic constraints A m(x, y, z) = 0."""
    for _ in range(steps):
        m, J = np.zeros(20), np.zeros((20, 3))
        x, y, z = xyz
        for k, (a, b, c) in enumerate(MONO):
            m[k] = x ** a * y ** b * z ** c
            J[k] = [a * x ** max(a - 1, 0) * y ** b * z ** c, b * x ** a * y ** max(b - 1, 0) * z ** c,
                    c * x ** a * y ** b * z ** max(c - 1, 0)]
        f, Jf = A @ m, A @ J
        try:
            d = np.linalg.solve(Jf.T @ Jf, -Jf.T @ f)
        except np.linalg.LinAlgError:
            break
        if not np.all(np.isfinite(d)):
            break
        xyz = xyz + d
    return xyz


def sampson(E, q1, q2):
    """EMEstimatorCallback::computeError: double arithmetic, float result."""
    E = np.asarray(E, np.float64)
    x1, y1, x2, y2 = q1[:, 0], q1[:, 1], q2[:, 0], q2[:, 1]
    ex0 = E[0, 0] * x1 + E[0, 1] * y1 + E[0, 2]
    ex1 = E[1, 0] * x1 + E[1, 1] * y1 + E[1, 2]
    ex2 = E[2, 0] * x1 + E[2, 1] * y1 + E[2, 2]
    et0 = E[0, 0] * x2 + E[1, 0] * y2 + E[2, 0]
    et1 = E[0, 1] * x2 + E[1, 1] * y2 + E[2, 1]
    d = x2 * ex0 + y2 * ex1 + ex2
    return (d * d / (ex0 * ex0 + ex1 * ex1 + et0 * et0 + et1 * et1)).astype(np.float32)


def threshold_sq(threshold, K4):
    t = threshold / ((float(K4[0]) + float(K4[1])) / 2)
    return np.float32(t * t)


def find_essential(p1, p2, K4, threshold=1.0, confidence=0.99, max_iters=1000, seed=0):
    """-> (models m x 3 x 3, mask, inlier count, iterations run), as svo_find_essential."""
    q1, q2 = normalise(p1, K4), normalise(p2, K4)
    n = len(q1)
    thr = threshold_sq(threshold, K4)
    mask = np.zeros(n, np.uint8)
    if n < 5:
        return np.zeros((0, 3, 3)), mask, 0, 0
    if n == 5:
        sols = five_point(q1, q2)
        return sols, np.full(n, 1 if len(sols) else 0, np.uint8), 5 if len(sols) else 0, 0
    niters, best, best_count, it = max_iters, None, 0, 0
    while it < niters:
        ok, idx = draw(n, seed, it)
        if not ok:
            break
        for E in five_point(q1[idx], q2[idx]):
            c = int((sampson(E, q1, q2) <= thr).sum())
            if c > max(best_count, 4):
                best, best_count = E, c
                niters = update_num_iters(confidence, (n - c) / n, 5, niters)
        it += 1
    if best is None:
        return np.zeros((0, 3, 3)), mask, 0, it
    mask = (sampson(best, q1, q2) <= thr).astype(np.uint8)
    return best[None], mask, best_count, it


def decompose(E):
    """decomposeEssentialMat with essential.hip's sign rule -> (R1, R2, t)."""
    U, _, Vt = np.linalg.svd(np.asarray(E, np.float64).reshape(3, 3))
    u, v = [U[:, 0].copy(), U[:, 1].copy()], [Vt[0].copy(), Vt[1].copy()]
    for k in range(2):
        if v[k][int(np.argmax(np.abs(v[k])))] < 0:
            u[k], v[k] = -u[k], -v[k]
    u2, v2 = np.cross(u[0], u[1]), np.cross(v[0], v[1])
    Um, Vm = np.stack([u[0], u[1], u2], 1), np.stack([v[0], v[1], v2], 1)
    return Um @ W @ Vm.T, Um @ W.T @ Vm.T, u2


def candidate_masks(E, q1, q2, dist=50.0):
    R1, R2, t = decompose(E)
    P0 = np.hstack([np.eye(3), np.zeros((3, 1))])
    out = []
    for R, tt in ((R1, t), (R2, t), (R1, -t), (R2, -t)):
        P = np.hstack([R, tt[:, None]])
        A = np.stack([q1[:, :1] * P0[2] - P0[0], q1[:, 1:] * P0[2] - P0[1], q2[:, :1] * P[2] - P[0],
                      q2[:, 1:] * P[2] - P[1]], 1)
        Q = np.linalg.svd(A)[2][:, -1, :]
        with np.errstate(divide="ignore", invalid="ignore"):
            m = Q[:, 2] * Q[:, 3] > 0
            X = Q / Q[:, 3:4]
            m &= X[:, 2] < dist
            z2 = X @ P[2]
            m &= (z2 > 0) & (z2 < dist)
        out.append(((R, tt), m))
    return out


def recover_pose(E, p1, p2, K4, dist=50.0, mask=None):
    """-> (R, t, good, chosen mask), as svo_recover_pose."""
    q1, q2 = normalise(p1, K4), normalise(p2, K4)
    cands = candidate_masks(E, q1, q2, dist)
    if mask is not None:
        cands = [(rt, m & (np.asarray(mask) != 0)) for rt, m in cands]
    g = [int(m.sum()) for _, m in cands]
    if g[0] >= g[1] and g[0] >= g[2] and g[0] >= g[3]:
        k = 0
    elif g[1] >= g[0] and g[1] >= g[2] and g[1] >= g[3]:
        k = 1
    elif g[2] >= g[0] and g[2] >= g[1] and g[2] >= g[3]:
        k = 2
    else:
        k = 3
    (R, t), m = cands[k]
    return R, t, g[k], m.astype(np.uint8), g


def essential_from_pose(R, t):
    """E = [t]x R, unit norm, largest entry positive."""
    t = np.asarray(t, np.float64)
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    return sign_fix(tx @ np.asarray(R, np.float64))


def push_off_epipolar(p1, p2, K4, R, t, dist_px, rows):
    """p2 with the given rows moved by dist_px pixels across their epipolar lines (outliers of a known distance)."""
    fx, fy, cx, cy = K4
    Ki = np.linalg.inv(np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]]))
    F = Ki.T @ essential_from_pose(R, t) @ Ki
    p2 = np.array(p2, np.float64)
    h1 = np.c_[np.asarray(p1, np.float64)[rows], np.ones(len(rows))]
    line = h1 @ F.T
    nrm = line[:, :2] / np.linalg.norm(line[:, :2], axis=1, keepdims=True)
    p2[rows] += nrm * np.asarray(dist_px, np.float64).reshape(-1, 1)
    return p2


def constraint_residuals(E):
    """|det E| and max |2 E E^T E - tr(E E^T) E| of a unit-norm E."""
    E = np.asarray(E, np.float64)
    EEt = E @ E.T
    return abs(np.linalg.det(E)), np.abs(2 * EEt @ E - np.trace(EEt) * E).max()
