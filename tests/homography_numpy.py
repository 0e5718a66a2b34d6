"""numpy restatement of findHomography (RANSAC), decomposeHomographyMat and the planar two-view pose as
ros_stereo_slam_amd/csrc/homography.hip states them.  Blind to the library; float64 except where upstream is float.

OpenCV 3.2's recipe (fundam.cpp, ptsetreg.cpp, homography_decomp.cpp), with every choice that OpenCV leaves to its own
LAPACK-like code stated here:
  * samples: draw k of iteration i is the splitmix64-style hash of (seed, i, k) modulo n; a slot whose value an earlier
    slot holds is drawn again, at most 64 draws per sample; a sample that checkSubset rejects is drawn again with the
    draw counter carried on, at most 8 samples per iteration, after which the iteration scores no model (DEVIATION:
    OpenCV's getSubset tries 1000 times and then ends the loop).
  * checkSubset: for the triples (0,1,2), (1,2,3), (0,2,3), (0,1,3), c = dx1 dy2 - dy1 dx2 from the first point of the
    triple, in double; collinear when |c| <= FLT_EPSILON (|dx1| + |dy1| + |dx2| + |dy2|) (haveCollinearPoints's test);
    the sample passes when no triple is collinear in either image and (c > 0) is the same in both images for every
    triple.  DEVIATIONS: OpenCV tests only the three triples that hold the last point for collinearity, and also passes
    a sample whose four triples all flip (a mirrored plane).
  * the 4-point solve: per-axis normalisation as runKernel (mean; scale 4 / sum |v - mean|; a sum below DBL_EPSILON: no
    model), then the 8 x 8 system with h8 = 1 IN NORMALISED COORDINATES by Gaussian elimination with partial pivoting
    (the first row of the largest magnitude; a pivot <= 1e-10: no model), back-substitution, H = T2^-1 Hn T1, H / h8.
    DEVIATION: OpenCV takes the null vector of the 9 x 9 L^T L; the two agree whenever h8 != 0 in normalised coordinates.
  * the error: HomographyEstimatorCallback::computeError in float, inliers err <= (float)(threshold^2).
  * the loop: sequential, first-best-wins over count > max(best, 3), the bound from the oracle's orc_update_num_iters.
  * the refit over the loop's inliers: runKernel's normalisation (means; count / sum |v - mean|), L^T L (45 sums), its
    eigen-decomposition by cyclic Jacobi -- pairs (0,1), (0,2) .. (7,8); a pair is skipped when |apq| <= DBL_EPSILON
    sqrt(|app aqq|); theta = (aqq - app) / (2 apq), t = sign(theta) / (|theta| + sqrt(theta^2 + 1)), c = 1 / sqrt(t^2 + 1),
    s = c t; columns p, q of every row, then rows p, q of every column; at most 30 sweeps -- the eigenvector of the first
    smallest eigenvalue, de-normalised, H / h8.  No sign rule is needed: h8 = 1 fixes the sign.  A refit that fails keeps
    the loop's model.
  * the polish: HomographyRefineCallback's residuals and Jacobian on h0 .. h7.  lambda = 1e-3; a step solves
    (J^T J + lambda diag(J^T J)) d = -J^T r by Cholesky; the step is taken when the cost falls (lambda / 10), otherwise
    dropped (lambda * 10); at most 10 steps; stop when max |d| <= 1e-12 max(1, max |h|) or the factorisation fails.
    DEVIATION: OpenCV's LMSolver keeps another schedule for lambda (gain ratio, lambda halved or multiplied by nu).
  * the summation tree of every sum over the inliers: thread t of 256 adds pairs t, t + 256, .. in order (a pair that is
    no inlier adds nothing); inside each group of 64 threads a butterfly x = x + x[lane ^ m], m = 1, 2 .. 32; the four
    group totals as ((w0 + w1) + w2) + w3.
  * the decomposition: Hn = K^-1 H K, negated when det Hn < 0, scaled so that the middle eigenvalue of Hn^T Hn (the
    same Jacobi, 3 x 3) is 1; lambda1 >= 1 >= lambda3 with v1, v2, v3;
    u = (sqrt(1 - lambda3) v1 +- sqrt(lambda1 - 1) v3) / sqrt(lambda1 - lambda3); U = [v2, u, v2 x u],
    W = [Hn v2, Hn u, Hn v2 x Hn u], R = W U^T, n = v2 x u, t = (Hn - R) n.  LABELLING: of (t, n) and (-t, -n) the
    first has nz > 0 (nz = 0: ny > 0; then nx > 0); `a` is the solution whose first normal is the larger by
    (nz, ny, nx); order (Ra, ta, na), (Ra, -ta, -na), (Rb, tb, nb), (Rb, -tb, -nb).  lambda1 - lambda3 <= 1e-8: a pure
    rotation, one solution, R = Hn V diag(lambda^-1/2) V^T, t = 0, n = (0, 0, 1).
  * the pose: every candidate scored by recoverPose's test with [R | t / |t|] (the DLT per pair by numpy's SVD), the
    first candidate with the largest count.
"""
from __future__ import annotations

import ctypes as C
import math
import types

import numpy as np

FLT_EPSILON = float(np.finfo(np.float32).eps)
DBL_EPSILON = float(np.finfo(np.float64).eps)
MAX_ATTEMPTS, MAX_DRAWS = 8, 64
TRIPLES = ((0, 1, 2), (1, 2, 3), (0, 2, 3), (0, 1, 3))
PURE_ROTATION = 1e-8
M64 = (1 << 64) - 1


def update_num_iters(p, ep, model_points, max_iters):
    from oracle import orc

    f = orc.load().orc_update_num_iters
    f.argtypes = [C.c_double, C.c_double, C.c_int, C.c_int]
    f.restype = C.c_int
    return f(p, ep, model_points, max_iters)


# ---- samples ----
def rng_u32(seed, it, draw):
    z = (seed + 0x9E3779B97F4A7C15 * (((it << 32) | draw) + 1)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z >> 32


def draw_distinct(seed, it, n, draw, m=4):
    """-> (filled, indices, the draw counter after)"""
    idx, guard, filled = [], 0, True
    for _ in range(m):
        v, got = 0, False
        while not got and guard < MAX_DRAWS:
            v = rng_u32(seed, it, draw) % n
            draw += 1
            guard += 1
            got = v not in idx
        filled = filled and got
        idx.append(v)
    return filled, idx, draw


def check_subset(a, b):
    """a, b: (.., 4, 2) float64 -> bool (..)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    ok = np.ones(a.shape[:-2], bool)
    for i, j, k in TRIPLES:
        cs = []
        for p in (a, b):
            dx1, dy1 = p[..., j, 0] - p[..., i, 0], p[..., j, 1] - p[..., i, 1]
            dx2, dy2 = p[..., k, 0] - p[..., i, 0], p[..., k, 1] - p[..., i, 1]
            c = dx1 * dy2 - dy1 * dx2
            ok &= ~(np.abs(c) <= FLT_EPSILON * (np.abs(dx1) + np.abs(dy1) + np.abs(dx2) + np.abs(dy2)))
            cs.append(c)
        ok &= (cs[0] > 0) == (cs[1] > 0)
    return ok


def sample(p1, p2, seed, it):
    """the 4-sample of iteration `it` -> (status, indices): 1 a sample that passed checkSubset, 0 every attempt rejected,
    -1 a slot could not be filled"""
    n, draw, idx = len(p1), 0, [0, 1, 2, 3]
    for _ in range(MAX_ATTEMPTS):
        filled, idx, draw = draw_distinct(seed, it, n, draw)
        if not filled:
            return -1, idx
        if check_subset(p1[idx].astype(np.float64), p2[idx].astype(np.float64)):
            return 1, idx
    return 0, idx


# ---- the minimal solve ----
def _axis4(v):
    c = (((v[:, 0] + v[:, 1]) + v[:, 2]) + v[:, 3]) / 4.0
    d = ((np.abs(v[:, 0] - c) + np.abs(v[:, 1] - c)) + np.abs(v[:, 2] - c)) + np.abs(v[:, 3] - c)
    return c, 4.0 / d, d >= DBL_EPSILON


def denormalise(g, c1, s1, c2, s2):
    """g: (B, 9); c, s: pairs of (B,) -> H (B, 9) with h8 = 1, ok"""
    g = g.reshape(-1, 3, 3)
    T = np.empty_like(g)
    T[:, :, 0] = g[:, :, 0] * s1[0][:, None]
    T[:, :, 1] = g[:, :, 1] * s1[1][:, None]
    T[:, :, 2] = g[:, :, 0] * (-c1[0] * s1[0])[:, None] + g[:, :, 1] * (-c1[1] * s1[1])[:, None] + g[:, :, 2]
    G = np.empty_like(g)
    G[:, 0] = T[:, 0] / s2[0][:, None] + c2[0][:, None] * T[:, 2]
    G[:, 1] = T[:, 1] / s2[1][:, None] + c2[1][:, None] * T[:, 2]
    G[:, 2] = T[:, 2]
    w = G[:, 2, 2]
    H = (G / w[:, None, None]).reshape(-1, 9)
    return H, (np.abs(w) > 0) & np.all(np.isfinite(H), 1)


def solve_4pt(x1, x2):
    """B samples (B x 4 x 2 each, x2 ~ H x1) -> (H: B x 9 with h8 = 1, zero where not ok; ok: B bool)"""
    a, b = np.asarray(x1, np.float64).reshape(-1, 4, 2), np.asarray(x2, np.float64).reshape(-1, 4, 2)
    B = len(a)
    with np.errstate(all="ignore"):
        ok = check_subset(a, b)
        c1x, s1x, o1 = _axis4(a[:, :, 0])
        c1y, s1y, o2 = _axis4(a[:, :, 1])
        c2x, s2x, o3 = _axis4(b[:, :, 0])
        c2y, s2y, o4 = _axis4(b[:, :, 1])
        ok &= o1 & o2 & o3 & o4
        M = np.zeros((B, 8, 9))
        for i in range(4):
            X, Y = (a[:, i, 0] - c1x) * s1x, (a[:, i, 1] - c1y) * s1y
            x, y = (b[:, i, 0] - c2x) * s2x, (b[:, i, 1] - c2y) * s2y
            M[:, 2 * i, 0], M[:, 2 * i, 1], M[:, 2 * i, 2] = X, Y, 1.0
            M[:, 2 * i, 6], M[:, 2 * i, 7], M[:, 2 * i, 8] = -x * X, -x * Y, x
            M[:, 2 * i + 1, 3], M[:, 2 * i + 1, 4], M[:, 2 * i + 1, 5] = X, Y, 1.0
            M[:, 2 * i + 1, 6], M[:, 2 * i + 1, 7], M[:, 2 * i + 1, 8] = -y * X, -y * Y, y
        rows = np.arange(B)
        for k in range(8):
            col = np.abs(M[:, k:, k])
            col = np.where(np.isnan(col), -1.0, col)
            p = np.argmax(col, 1) + k
            ok &= col[rows, p - k] > 1e-10
            rk, rp = M[rows, k].copy(), M[rows, p].copy()
            M[rows, k], M[rows, p] = rp, rk
            for r in range(k + 1, 8):
                f = M[:, r, k] / M[:, k, k]
                M[:, r, k + 1:] -= f[:, None] * M[:, k, k + 1:]
        g = np.ones((B, 9))
        for k in range(7, -1, -1):
            acc = M[:, k, 8].copy()
            for c in range(k + 1, 8):
                acc -= M[:, k, c] * g[:, c]
            g[:, k] = acc / M[:, k, k]
        H, fin = denormalise(g, (c1x, c1y), (s1x, s1y), (c2x, c2y), (s2x, s2y))
        ok &= fin
    H[~ok] = 0.0
    return H, ok


def transfer_error(H, p1, p2):
    """HomographyEstimatorCallback::computeError, float throughout.  H: (m, 9) or (9,); -> (m, n) or (n,) float32"""
    Hf = np.asarray(H, np.float64).reshape(-1, 9).astype(np.float32)[:, :, None]
    p1, p2 = np.asarray(p1, np.float32), np.asarray(p2, np.float32)
    X, Y, x, y = p1[None, :, 0], p1[None, :, 1], p2[None, :, 0], p2[None, :, 1]
    one = np.float32(1)
    with np.errstate(all="ignore"):
        ww = one / (Hf[:, 6] * X + Hf[:, 7] * Y + one)
        dx = (Hf[:, 0] * X + Hf[:, 1] * Y + Hf[:, 2]) * ww - x
        dy = (Hf[:, 3] * X + Hf[:, 4] * Y + Hf[:, 5]) * ww - y
        e = dx * dx + dy * dy
    return e[0] if np.ndim(H) == 1 else e


# ---- sums over the inliers ----
def tree_sum(terms):
    """terms: (n, K), zero rows for pairs that are no inliers -> (K,) in block_sum's order"""
    n, K = terms.shape
    rows = max(1, -(-n // 256))
    T = np.zeros((rows * 256, K))
    T[:n] = terms
    T = T.reshape(rows, 256, K)
    acc = np.zeros((256, K))
    for r in range(rows):
        acc = acc + T[r]
    x = acc.reshape(4, 64, K)
    lanes = np.arange(64)
    for m in (1, 2, 4, 8, 16, 32):
        x = x + x[:, lanes ^ m]
    w = x[:, 0]
    return ((w[0] + w[1]) + w[2]) + w[3]


def jacobi_angle(app, aqq, apq):
    if apq == 0 or abs(apq) <= DBL_EPSILON * math.sqrt(abs(app * aqq)):
        return None
    theta = (aqq - app) / (2.0 * apq)
    t = (1.0 if theta >= 0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
    c = 1.0 / math.sqrt(t * t + 1.0)
    return c, c * t


def jacobi_sym(A):
    """-> (the rotated A, whose diagonal holds the eigenvalues; V, its columns the eigenvectors)"""
    A = np.array(A, np.float64)
    N = len(A)
    V = np.eye(N)
    for _ in range(30):
        rotated = False
        for p in range(N - 1):
            for q in range(p + 1, N):
                cs = jacobi_angle(float(A[p, p]), float(A[q, q]), float(A[p, q]))
                if cs is None:
                    continue
                rotated = True
                c, s = cs
                ap, aq = A[:, p].copy(), A[:, q].copy()
                A[:, p], A[:, q] = c * ap - s * aq, s * ap + c * aq
                ap, aq = A[p].copy(), A[q].copy()
                A[p], A[q] = c * ap - s * aq, s * ap + c * aq
                vp, vq = V[:, p].copy(), V[:, q].copy()
                V[:, p], V[:, q] = c * vp - s * vq, s * vp + c * vq
        if not rotated:
            break
    return A, V


def refit(P1, P2, inl):
    """the normalised DLT over the pairs with inl set (P1, P2 float64) -> H (9,) with h8 = 1, or None"""
    inl = np.asarray(inl, bool)
    z = inl[:, None].astype(np.float64)
    v5 = tree_sum(np.c_[np.ones(len(P1)), P1, P2] * z)
    cnt = v5[0]
    c1, c2 = v5[1:3] / cnt, v5[3:5] / cnt
    v4 = tree_sum(np.c_[np.abs(P1 - c1), np.abs(P2 - c2)] * z)
    if not np.all(v4 >= DBL_EPSILON):
        return None
    s1, s2 = cnt / v4[:2], cnt / v4[2:]
    X, Y = (P1[:, 0] - c1[0]) * s1[0], (P1[:, 1] - c1[1]) * s1[1]
    x, y = (P2[:, 0] - c2[0]) * s2[0], (P2[:, 1] - c2[1]) * s2[1]
    o, zz = np.ones_like(X), np.zeros_like(X)
    Lx = np.stack([X, Y, o, zz, zz, zz, -x * X, -x * Y, -x], 1)
    Ly = np.stack([zz, zz, zz, X, Y, o, -y * X, -y * Y, -y], 1)
    terms = np.stack([Lx[:, j] * Lx[:, k] + Ly[:, j] * Ly[:, k] for j in range(9) for k in range(j, 9)], 1)
    acc = tree_sum(np.where(inl[:, None], terms, 0.0))
    LtL = np.zeros((9, 9))
    m = 0
    for j in range(9):
        for k in range(j, 9):
            LtL[j, k] = LtL[k, j] = acc[m]
            m += 1
    D, V = jacobi_sym(LtL)
    g = V[:, int(np.argmin(np.diag(D)))]
    one = lambda v: (np.array([v[0]]), np.array([v[1]]))  # noqa: E731
    with np.errstate(all="ignore"):
        H, ok = denormalise(g[None].copy(), one(c1), one(s1), one(c2), one(s2))
    return H[0] if ok[0] else None


def lm_sums(h, P1, P2, inl):
    """J^T J (36, upper triangle by rows), J^T r (8) and the cost at h (8,), in the tree's order"""
    X, Y, x, y = P1[:, 0], P1[:, 1], P2[:, 0], P2[:, 1]
    with np.errstate(all="ignore"):
        ww = h[6] * X + h[7] * Y + 1.0
        ww = np.where(np.abs(ww) > DBL_EPSILON, 1.0 / ww, 0.0)
        xi, yi = (h[0] * X + h[1] * Y + h[2]) * ww, (h[3] * X + h[4] * Y + h[5]) * ww
        rx, ry = xi - x, yi - y
        zz = np.zeros_like(X)
        J0 = [X * ww, Y * ww, ww, zz, zz, zz, -X * ww * xi, -Y * ww * xi]
        J1 = [zz, zz, zz, X * ww, Y * ww, ww, -X * ww * yi, -Y * ww * yi]
        cols = [J0[j] * J0[k] + J1[j] * J1[k] for j in range(8) for k in range(j, 8)]
        cols += [J0[j] * rx + J1[j] * ry for j in range(8)]
        cols.append(rx * rx + ry * ry)
        return tree_sum(np.where(np.asarray(inl, bool)[:, None], np.stack(cols, 1), 0.0))


def _tri8(j, k):
    return j * 8 - j * (j - 1) // 2 + (k - j)


def lm_step(acc, lam):
    """(A + lam diag A) d = -g by Cholesky -> d (8,) or None"""
    a = [float(v) for v in acc]
    L = [[0.0] * 8 for _ in range(8)]
    for j in range(8):
        for i in range(j, 8):
            s = a[_tri8(j, j)] + lam * a[_tri8(j, j)] if i == j else a[_tri8(j, i)]
            for k in range(j):
                s -= L[i][k] * L[j][k]
            if i == j:
                if not s > 0:
                    return None
                L[j][j] = math.sqrt(s)
            else:
                L[i][j] = s / L[j][j]
    yv = [0.0] * 8
    for i in range(8):
        s = -a[36 + i]
        for k in range(i):
            s -= L[i][k] * yv[k]
        yv[i] = s / L[i][i]
    d = [0.0] * 8
    for i in range(7, -1, -1):
        s = yv[i]
        for k in range(i + 1, 8):
            s -= L[k][i] * d[k]
        d[i] = s / L[i][i]
    return np.array(d) if all(math.isfinite(v) for v in d) else None


def polish(H, P1, P2, inl, steps=10):
    h = np.array(H[:8], np.float64)
    acc = lm_sums(h, P1, P2, inl)
    lam = 1e-3
    for _ in range(steps):
        d = lm_step(acc, lam)
        if d is None:
            break
        ht = h + d
        acct = lm_sums(ht, P1, P2, inl)
        if acct[44] < acc[44]:
            h, acc = ht, acct
            lam *= 0.1
        else:
            lam *= 10.0
        if np.abs(d).max() <= 1e-12 * max(1.0, np.abs(h).max()):
            break
    return np.r_[h, 1.0]


def refit_polish(H, P1, P2, inl):
    """the refit over the inliers (kept when it succeeds) and the polish; P1, P2 float64"""
    P1, P2 = np.asarray(P1, np.float64), np.asarray(P2, np.float64)
    Hr = refit(P1, P2, inl)
    return polish(H if Hr is None else Hr, P1, P2, inl)


# ---- the loop ----
def find_homography(p1, p2, threshold=3.0, confidence=0.995, max_iters=2000, seed=0):
    """-> namespace(H (3 x 3, zero without a model), mask, count, iters, margin_ok, H_loop), as svo_find_homography.
    margin_ok: no pair's float error lies within 1e-6 relative of threshold^2 for any model the sequential loop scores."""
    p1, p2 = np.asarray(p1, np.float32).reshape(-1, 2), np.asarray(p2, np.float32).reshape(-1, 2)
    n = len(p1)
    thr = np.float32(threshold * threshold)
    out = types.SimpleNamespace(H=np.zeros((3, 3)), mask=np.zeros(n, np.uint8), count=0, iters=0, margin_ok=True, H_loop=None)
    if n < 4:
        return out
    if n == 4:
        H, ok = solve_4pt(p1.astype(np.float64)[None], p2.astype(np.float64)[None])
        if ok[0]:
            out.H, out.mask, out.count, out.H_loop = H[0].reshape(3, 3), np.ones(4, np.uint8), 4, H[0]
        return out
    niters, best, best_count, it, stopped = max_iters, None, 0, 0, False
    bounds = [0, 64, 256] + list(range(512, max_iters, 256)) + [max_iters]
    for c0, c1 in zip(bounds[:-1], bounds[1:]):
        c1 = min(c1, niters, max_iters)
        if stopped or c0 >= c1 or it < c0:
            break
        st = [sample(p1, p2, seed, i) for i in range(c0, c1)]
        idx = np.array([s[1] for s in st])
        H, ok = solve_4pt(p1[idx].astype(np.float64), p2[idx].astype(np.float64))
        ok &= np.array([s[0] == 1 for s in st])
        err = transfer_error(H, p1, p2)
        counts = (err <= thr).sum(1)
        near = (np.abs(err.astype(np.float64) - float(thr)) <= 1e-6 * float(thr)).any(1)
        while it < c1 and it < niters:
            k = it - c0
            if st[k][0] < 0:
                stopped = True
                break
            if ok[k]:
                out.margin_ok = out.margin_ok and not near[k]
                c = int(counts[k])
                if c > max(best_count, 3):
                    best, best_count = H[k].copy(), c
                    niters = update_num_iters(confidence, (n - c) / n, 4, niters)
            it += 1
    out.iters = it
    if best is None:
        return out
    out.H_loop = best
    out.mask = (transfer_error(best, p1, p2) <= thr).astype(np.uint8)
    out.count = best_count
    out.H = refit_polish(best, p1, p2, out.mask != 0).reshape(3, 3)
    return out


# ---- the decomposition ----
def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def decompose(H, K4):
    """-> list of (R, t, n), as svo_decompose_homography (0, 1 or 4 of them)"""
    h = [float(v) for v in np.asarray(H, np.float64).reshape(9)]
    fx, fy, cx, cy = (float(v) for v in K4)
    A = [[h[3 * i] * fx, h[3 * i + 1] * fy, h[3 * i] * cx + h[3 * i + 1] * cy + h[3 * i + 2]] for i in range(3)]
    Hn = [[(A[0][j] - cx * A[2][j]) / fx for j in range(3)], [(A[1][j] - cy * A[2][j]) / fy for j in range(3)], list(A[2])]
    det = (Hn[0][0] * (Hn[1][1] * Hn[2][2] - Hn[1][2] * Hn[2][1]) - Hn[0][1] * (Hn[1][0] * Hn[2][2] - Hn[1][2] * Hn[2][0])
           + Hn[0][2] * (Hn[1][0] * Hn[2][1] - Hn[1][1] * Hn[2][0]))
    if not abs(det) > 0 or not math.isfinite(det):
        return []
    S = np.zeros((3, 3))
    for i in range(3):
        for j in range(i, 3):
            S[i, j] = S[j, i] = Hn[0][i] * Hn[0][j] + Hn[1][i] * Hn[1][j] + Hn[2][i] * Hn[2][j]
    D, V = jacobi_sym(S)
    lam = [float(D[i, i]) for i in range(3)]
    o = [0, 1, 2]
    for i in range(1, 3):
        j = i
        while j > 0 and lam[o[j]] > lam[o[j - 1]]:
            o[j], o[j - 1] = o[j - 1], o[j]
            j -= 1
    l2 = lam[o[1]]
    if not l2 > 0 or not math.isfinite(l2):
        return []
    sc = (-1.0 if det < 0 else 1.0) / math.sqrt(l2)
    Hn = [[v * sc for v in row] for row in Hn]
    l1, l3 = lam[o[0]] / l2, lam[o[2]] / l2
    v1, v2, v3 = ([float(V[i, o[m]]) for i in range(3)] for m in range(3))
    if not l3 > 0 or not math.isfinite(l1):
        return []
    if l1 - l3 <= PURE_ROTATION:
        w, v = [1.0 / math.sqrt(l1), 1.0, 1.0 / math.sqrt(l3)], [v1, v2, v3]
        R = np.zeros((3, 3))
        for i in range(3):
            for j in range(3):
                r = 0.0
                for m in range(3):
                    hv = Hn[i][0] * v[m][0] + Hn[i][1] * v[m][1] + Hn[i][2] * v[m][2]
                    r += hv * w[m] * v[m][j]
                R[i, j] = r
        return [(R, np.zeros(3), np.array([0.0, 0.0, 1.0]))]
    ca, cb, den = math.sqrt(max(1.0 - l3, 0.0)), math.sqrt(max(l1 - 1.0, 0.0)), math.sqrt(l1 - l3)
    sols = []
    for sg in (1.0, -1.0):
        u = [(ca * v1[i] + sg * cb * v3[i]) / den for i in range(3)]
        N = _cross(v2, u)
        hv = [Hn[i][0] * v2[0] + Hn[i][1] * v2[1] + Hn[i][2] * v2[2] for i in range(3)]
        hu = [Hn[i][0] * u[0] + Hn[i][1] * u[1] + Hn[i][2] * u[2] for i in range(3)]
        hn = _cross(hv, hu)
        R = [[hv[i] * v2[j] + hu[i] * u[j] + hn[i] * N[j] for j in range(3)] for i in range(3)]
        flip = N[2] < 0 if N[2] != 0 else (N[1] < 0 if N[1] != 0 else N[0] < 0)
        T = [(Hn[i][0] - R[i][0]) * N[0] + (Hn[i][1] - R[i][1]) * N[1] + (Hn[i][2] - R[i][2]) * N[2] for i in range(3)]
        sgn = -1.0 if flip else 1.0
        sols.append((np.array(R), np.array([sgn * v for v in T]), np.array([sgn * v for v in N])))
    na, nb = sols[0][2], sols[1][2]
    first = (na[2] > nb[2]) if na[2] != nb[2] else ((na[1] > nb[1]) if na[1] != nb[1] else bool(na[0] >= nb[0]))
    if not first:
        sols = sols[::-1]
    return [(sols[0][0], sols[0][1], sols[0][2]), (sols[0][0], -sols[0][1], -sols[0][2]),
            (sols[1][0], sols[1][1], sols[1][2]), (sols[1][0], -sols[1][1], -sols[1][2])]


def normalised_h(H, K4):
    """Hn = K^-1 H K with det > 0 and middle singular value 1 (by numpy's SVD: for checking decompositions)"""
    fx, fy, cx, cy = K4
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
    Hn = np.linalg.inv(K) @ np.asarray(H, np.float64).reshape(3, 3) @ K
    Hn = Hn * np.sign(np.linalg.det(Hn))
    return Hn / np.linalg.svd(Hn, compute_uv=False)[1]


# ---- the pose ----
def normalise(p, K4):
    fx, fy, cx, cy = (float(v) for v in K4)
    p = np.asarray(p, np.float32).reshape(-1, 2).astype(np.float64)
    return np.stack([(p[:, 0] - cx) / fx, (p[:, 1] - cy) / fy], 1)


def unit(t):
    nn = math.sqrt(float(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]))
    return t / nn if nn > 0 else np.zeros(3)


def candidate_mask(R, t, q1, q2, dist):
    P0 = np.hstack([np.eye(3), np.zeros((3, 1))])
    P = np.hstack([R, t[:, None]])
    A = np.stack([q1[:, :1] * P0[2] - P0[0], q1[:, 1:] * P0[2] - P0[1], q2[:, :1] * P[2] - P[0], q2[:, 1:] * P[2] - P[1]], 1)
    Q = np.linalg.svd(A)[2][:, -1, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        m = Q[:, 2] * Q[:, 3] > 0
        X = Q / Q[:, 3:4]
        m &= X[:, 2] < dist
        z2 = X @ P[2]
        m &= (z2 > 0) & (z2 < dist)
    return m


def homography_pose(H, p1, p2, K4, dist=50.0, mask=None):
    """-> (R, t, n, good4, the chosen candidate's mask), as svo_homography_pose"""
    q1, q2 = normalise(p1, K4), normalise(p2, K4)
    sols = decompose(H, K4)
    good4 = [0, 0, 0, 0]
    if not sols:
        return np.zeros((3, 3)), np.zeros(3), np.zeros(3), good4, np.zeros(len(q1), np.uint8)
    masks = []
    for k, (R, t, n) in enumerate(sols):
        m = candidate_mask(R, unit(t), q1, q2, dist)
        if mask is not None:
            m &= np.asarray(mask) != 0
        masks.append(m)
        good4[k] = int(m.sum())
    pick = 0
    for k in range(1, len(sols)):
        if good4[k] > good4[pick]:
            pick = k
    R, t, n = sols[pick]
    return R, unit(t), n, good4, masks[pick].astype(np.uint8)


def homography_from_pose(R, t, n, d, K4):
    """the pixel homography of the plane n . X = d (first camera's frame) under X2 = R X1 + t, h8 = 1"""
    fx, fy, cx, cy = K4
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
    H = K @ (np.asarray(R) + np.outer(t, n) / d) @ np.linalg.inv(K)
    return H / H[2, 2]
