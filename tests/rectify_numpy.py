"""numpy restatement of the rectification chain: stereoRectify -> initUndistortRectifyMap -> remap, and undistortPoints
(csrc/rectify.hip, csrc/rectify_plan.hip.h).  Nothing of OpenCV can run here, so every point is either
RECALLED (OpenCV 3.2 from memory) or OURS, and numbered.  Everything is double, in exactly the written operation order, no FMA.

 N1  (recalled) D holds 0, 4, 5 or 8 coefficients k1 k2 p1 p2 [k3 [k4 k5 k6]]; the missing ones are zero.  12 / 14 are refused.
 N2  (recalled) kr = (1 + ((k3 r2 + k2) r2 + k1) r2) / (1 + ((k6 r2 + k5) r2 + k4) r2); xd = x kr + p1 (2xy) + p2 (r2 + 2x^2);
     yd = y kr + p1 (r2 + 2y^2) + p2 (2xy); u = fx xd + cx; v = fy yd + cy.  2xy is formed as (2 x) y, 2x^2 as (2 x) x.
 N3  (recalled) Rodrigues: vector -> matrix R = c I + (1 - c) r r^T + s [r]x with r = v / theta, the identity below
     theta = DBL_EPSILON; matrix -> vector from the skew part, s = |skew| / 2, c = (trace - 1) / 2 clamped to [-1, 1],
     theta = acos(c), v = skew / (2 s) theta; s < 1e-5: zero for c > 0, the diagonal form for a half turn.
 N4  (ours)     the matrix -> vector form does not re-orthonormalise R by an SVD first: R is taken as a rotation.
 N5  (recalled) Bouguet's stereoRectify, steps 1 - 9 of the recipe (`stereo_rectify` below, commented step by step).
 N6  (recalled) the image corners are (0, 0), (w-1, 0), (0, h-1), (w-1, h-1) -- svo_stereo_rectify_q's choice (R15 of
     tests/sgbm_numpy.py) -- and upstream keeps them as FLOAT points after the undistortion and after the projection; so do we.
 N7  (recalled) with alpha = -1 a new image size changes neither P nor Q (it scales the principal points only for alpha >= 0).
 N8  (ours)     alpha >= 0 (inner / outer rectangles, valid ROIs) is refused.
 N9  (ours)     the inverse of P[:, :3] R is the adjugate over the determinant in the order of `inv3` (upstream: an LU solve).
 N10 (ours)     [X Y W] = iR [j i 1] as j iR[k][0] + (i iR[k][1] + iR[k][2]) per pixel (upstream: a running sum along the row), and
     x = X / W (upstream multiplies by 1 / W).
 N11 (recalled) fixed-point maps: iu = rint(u 32) (half to even), a NaN or a rounded magnitude of 2^31 or more gives INT_MIN;
     xy = (iu >> 5, iv >> 5) (arithmetic shift: floor), frac = (iv & 31) 32 + (iu & 31).
 N12 (ours)     xy saturates to int16 (upstream wraps): a far coordinate reads the border.
 N13 (recalled) undistortPoints: x0 = (u - cx) / fx, five iterations x <- (x0 - dx) icd with icd = 1 / kr and the tangential
     terms of N2 at the current (x, y); then [X Y W] = R [x y 1], x = X / W; with P: u = x P[0][0] + P[0][2], v = y P[1][1] + P[1][2].
 N14 (recalled) remap, INTER_LINEAR, BORDER_CONSTANT, uint8: weights 32 (32-a)(32-b), 32 a (32-b), 32 (32-a) b, 32 a b (the table
     at INTER_REMAP_COEF_SCALE 2^15, `cv_weight_table`), dst = (sum w p + 2^14) >> 15 per channel, every tap outside the source
     reads `value` (one byte for every channel).
 N15 (recalled) a float map pair is converted as N11 / N12 per coordinate: sx = rint(mapx 32), xy = sat16(sx >> 5), fraction sx & 31.
"""
import numpy as np

INT_MIN = -(1 << 31)


def coeffs(D):
    D = np.zeros(0) if D is None else np.asarray(D, np.float64).reshape(-1)
    if len(D) not in (0, 4, 5, 8):
        raise ValueError("D must hold 0, 4, 5 or 8 coefficients")
    k = np.zeros(8)
    k[:len(D)] = D
    return k  # k1 k2 p1 p2 k3 k4 k5 k6


def kr(r2, k):
    return (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2) / (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2)


def tangential(x, y, r2, k):
    a1 = (2 * x) * y
    return k[2] * a1 + k[3] * (r2 + (2 * x) * x), k[2] * (r2 + (2 * y) * y) + k[3] * a1


def distort(x, y, K, D):
    """N2: normalised (x, y) -> pixel (u, v), unrounded"""
    K, k = np.asarray(K, np.float64).reshape(3, 3), coeffs(D)
    r2 = x * x + y * y
    c = kr(r2, k)
    dx, dy = tangential(x, y, r2, k)
    return K[0, 0] * (x * c + dx) + K[0, 2], K[1, 1] * (y * c + dy) + K[1, 2]


def rodrigues(a):
    a = np.asarray(a, np.float64)
    if a.size == 3:
        v = a.reshape(3)
        theta = np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
        if theta < np.finfo(np.float64).eps:
            return np.eye(3)
        c, s = np.cos(theta), np.sin(theta)
        c1 = 1 - c
        r = v / theta
        rx = np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]])
        return c * np.eye(3) + c1 * np.outer(r, r) + s * rx
    R = a.reshape(3, 3)
    r = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = np.sqrt((r[0] * r[0] + r[1] * r[1] + r[2] * r[2]) * 0.25)
    c = min(max((R[0, 0] + R[1, 1] + R[2, 2] - 1) * 0.5, -1.0), 1.0)
    theta = np.arccos(c)
    if s < 1e-5:
        if c > 0:
            return np.zeros(3)
        r = np.array([np.sqrt(max((R[0, 0] + 1) * 0.5, 0.0)),
                      np.sqrt(max((R[1, 1] + 1) * 0.5, 0.0)) * (-1.0 if R[0, 1] < 0 else 1.0),
                      np.sqrt(max((R[2, 2] + 1) * 0.5, 0.0)) * (-1.0 if R[0, 2] < 0 else 1.0)])
        if abs(r[0]) < abs(r[1]) and abs(r[0]) < abs(r[2]) and (R[1, 2] > 0) != (r[1] * r[2] > 0):
            r[2] = -r[2]
        return r * (theta / np.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]))
    return r * ((1 / (2 * s)) * theta)


def mat3(A, B):
    """3 x 3 product, every entry (a0 b0 + a1 b1) + a2 b2"""
    A, B = np.asarray(A, np.float64).reshape(3, 3), np.asarray(B, np.float64).reshape(3, -1)
    out = np.zeros((3, B.shape[1]))
    for r in range(3):
        for c in range(B.shape[1]):
            out[r, c] = (A[r, 0] * B[0, c] + A[r, 1] * B[1, c]) + A[r, 2] * B[2, c]
    return out


def inv3(M):
    """N9"""
    m = np.asarray(M, np.float64).reshape(3, 3)
    c00 = m[1, 1] * m[2, 2] - m[1, 2] * m[2, 1]
    c01 = m[1, 2] * m[2, 0] - m[1, 0] * m[2, 2]
    c02 = m[1, 0] * m[2, 1] - m[1, 1] * m[2, 0]
    det = (m[0, 0] * c00 + m[0, 1] * c01) + m[0, 2] * c02
    adj = np.array([[c00, m[0, 2] * m[2, 1] - m[0, 1] * m[2, 2], m[0, 1] * m[1, 2] - m[0, 2] * m[1, 1]],
                    [c01, m[0, 0] * m[2, 2] - m[0, 2] * m[2, 0], m[0, 2] * m[1, 0] - m[0, 0] * m[1, 2]],
                    [c02, m[0, 1] * m[2, 0] - m[0, 0] * m[2, 1], m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]]])
    return adj / det


def undistort_points(pts, K, D, R=None, P=None, iters=5):
    """N13 -> float64 [n, 2] (the float entry point rounds this once to float32); pts: float32 values"""
    pts = np.asarray(pts, np.float32).reshape(-1, 2).astype(np.float64)
    K, k = np.asarray(K, np.float64).reshape(3, 3), coeffs(D)
    x0, y0 = (pts[:, 0] - K[0, 2]) / K[0, 0], (pts[:, 1] - K[1, 2]) / K[1, 1]
    x, y = x0.copy(), y0.copy()
    for _ in range(iters):
        r2 = x * x + y * y
        icd = 1.0 / kr(r2, k)
        dx, dy = tangential(x, y, r2, k)
        x, y = (x0 - dx) * icd, (y0 - dy) * icd
    if R is not None:
        R = np.asarray(R, np.float64).reshape(3, 3)
        X = (R[0, 0] * x + R[0, 1] * y) + R[0, 2]
        Y = (R[1, 0] * x + R[1, 1] * y) + R[1, 2]
        W = (R[2, 0] * x + R[2, 1] * y) + R[2, 2]
        x, y = X / W, Y / W
    if P is not None:
        P = np.asarray(P, np.float64).reshape(3, -1)
        x, y = x * P[0, 0] + P[0, 2], y * P[1, 1] + P[1, 2]
    return np.stack([x, y], 1)


CALIB_ZERO_DISPARITY = 1024


def stereo_rectify(K1, D1, K2, D2, size, R, T, flags=CALIB_ZERO_DISPARITY, alpha=-1.0, new_size=None):
    """N5 -> (R1, R2, P1, P2, Q)"""
    if alpha != -1:
        raise ValueError("alpha >= 0 is not built (N8)")
    w, h = size
    Ks = [np.asarray(K1, np.float64).reshape(3, 3), np.asarray(K2, np.float64).reshape(3, 3)]
    Ds = [coeffs(D1), coeffs(D2)]
    R, T = np.asarray(R, np.float64).reshape(3, 3), np.asarray(T, np.float64).reshape(3)
    # 1. each camera takes half the rotation
    r_r = rodrigues(rodrigues(R) * -0.5)
    t = mat3(r_r, T)[:, 0]
    # 2. the axis the baseline lies along
    idx = 0 if abs(t[0]) > abs(t[1]) else 1
    c = t[idx]
    nt = np.sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2])
    uu = np.zeros(3)
    uu[idx] = 1.0 if c > 0 else -1.0
    # 3. the rotation that turns the baseline onto that axis
    ww = np.array([t[1] * uu[2] - t[2] * uu[1], t[2] * uu[0] - t[0] * uu[2], t[0] * uu[1] - t[1] * uu[0]])
    nw = np.sqrt(ww[0] * ww[0] + ww[1] * ww[1] + ww[2] * ww[2])
    if nw > 0:
        ww = ww * (np.arccos(abs(c) / nt) / nw)
    wR = rodrigues(ww)
    # 4.
    R1, R2 = mat3(wR, r_r.T), mat3(wR, r_r)
    t = mat3(R2, T)[:, 0]
    # 5. the new focal length
    fc_new = np.inf
    for K, k in zip(Ks, Ds):
        fc = K[idx ^ 1, idx ^ 1]
        if k[0] < 0:
            fc = fc * (1 + k[0] * (w * w + h * h) / (4 * fc * fc))
        fc_new = min(fc_new, fc)
    # 6. the principal points from the undistorted, rotated corners (N6: float points at both stages)
    corners = np.array([[0, 0], [w - 1, 0], [0, h - 1], [w - 1, h - 1]], np.float32)
    cc = np.zeros((2, 2))
    for n, (K, k, Ri) in enumerate(zip(Ks, Ds, (R1, R2))):
        nrm = undistort_points(corners, K, k).astype(np.float32).astype(np.float64)
        X = (Ri[0, 0] * nrm[:, 0] + Ri[0, 1] * nrm[:, 1]) + Ri[0, 2]
        Y = (Ri[1, 0] * nrm[:, 0] + Ri[1, 1] * nrm[:, 1]) + Ri[1, 2]
        W = (Ri[2, 0] * nrm[:, 0] + Ri[2, 1] * nrm[:, 1]) + Ri[2, 2]
        px = ((X / W) * fc_new + 0.0).astype(np.float32).astype(np.float64)
        py = ((Y / W) * fc_new + 0.0).astype(np.float32).astype(np.float64)
        sx = ((px[0] + px[1]) + px[2]) + px[3]
        sy = ((py[0] + py[1]) + py[2]) + py[3]
        cc[n] = (w - 1) / 2.0 - sx * 0.25, (h - 1) / 2.0 - sy * 0.25
    # 7.
    if flags & CALIB_ZERO_DISPARITY:
        cc[0] = cc[1] = (cc[0] + cc[1]) * 0.5
    else:
        cc[0, idx ^ 1] = cc[1, idx ^ 1] = (cc[0, idx ^ 1] + cc[1, idx ^ 1]) * 0.5
    # 8. / 9.
    P1, P2 = np.zeros((3, 4)), np.zeros((3, 4))
    for P, c2 in ((P1, cc[0]), (P2, cc[1])):
        P[0, 0] = P[1, 1] = fc_new
        P[0, 2], P[1, 2], P[2, 2] = c2[0], c2[1], 1.0
    P2[idx, 3] = t[idx] * fc_new
    Q = np.zeros((4, 4))
    Q[0, 0] = Q[1, 1] = 1.0
    Q[0, 3], Q[1, 3], Q[2, 3] = -cc[0, 0], -cc[0, 1], fc_new
    Q[3, 2] = -1.0 / t[idx]
    Q[3, 3] = (cc[0, idx] - cc[1, idx]) / t[idx]
    return R1, R2, P1, P2, Q


def rectify_uv(K, D, R, P, size):
    """N9, N10, N2: the unrounded source coordinate (u, v) of every pixel of the rectified image, [h, w] float64 each"""
    w, h = size
    K = np.asarray(K, np.float64).reshape(3, 3)
    Pm = K if P is None else np.asarray(P, np.float64).reshape(3, -1)[:, :3]
    iR = inv3(Pm if R is None else mat3(Pm, R))
    j, i = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    X = j * iR[0, 0] + (i * iR[0, 1] + iR[0, 2])
    Y = j * iR[1, 0] + (i * iR[1, 1] + iR[1, 2])
    W = j * iR[2, 0] + (i * iR[2, 1] + iR[2, 2])
    with np.errstate(all="ignore"):
        return distort(X / W, Y / W, K, D)


def fix5(v):
    """N11: rint(v 32) as x86's cvtsd2si gives it, int64 holding an int32 value"""
    with np.errstate(all="ignore"):
        r = np.rint(np.asarray(v, np.float64) * 32)
        ok = (r >= -2147483648.0) & (r < 2147483648.0)
    return np.where(ok, np.where(ok, r, 0), INT_MIN).astype(np.int64)


def fixed_maps(u, v):
    """N11, N12 -> (xy int16 [h, w, 2], frac uint16 [h, w])"""
    iu, iv = fix5(u), fix5(v)
    xy = np.stack([np.clip(iu >> 5, -32768, 32767), np.clip(iv >> 5, -32768, 32767)], -1).astype(np.int16)
    return xy, ((iv & 31) * 32 + (iu & 31)).astype(np.uint16)


def init_undistort_rectify_map(K, D, R, P, size):
    return fixed_maps(*rectify_uv(K, D, R, P, size))


def float_maps(mapx, mapy):
    """N15: float32 maps; the product by 32 is exact in double"""
    return fixed_maps(np.asarray(mapx, np.float32).astype(np.float64), np.asarray(mapy, np.float32).astype(np.float64))


def cv_weight_table():
    """OpenCV's initInterTab2D(INTER_LINEAR, fixpt) restated literally -> int [1024, 4] (taps (0,0) (0,1) (1,0) (1,1) of fraction
    fy 32 + fx) and the fractions at which its sum correction changed an entry.  It does so at one: fraction (0, 0), whose
    weight 2^15 saturate_cast<short> cuts to 32767 and the correction puts back (kept here as an int; as a weight of 32767 or of
    2^15 the pixel is the same for every byte: (32768 p + 16384 - p) >> 15 = p).  Everywhere else the weights are exact."""
    tab1 = np.zeros((32, 2), np.float32)
    scale = np.float32(1.0 / 32)
    for i in range(32):
        x = np.float32(i) * scale
        tab1[i] = np.float32(1) - x, x
    out, fired = np.zeros((1024, 4), np.int64), []
    for i in range(32):
        for j in range(32):
            fl = np.array([[tab1[i, k1] * tab1[j, k2] for k2 in range(2)] for k1 in range(2)], np.float32)
            it = np.clip(np.rint(fl.astype(np.float64) * 32768), -32768, 32767).astype(np.int64)  # saturate_cast<short>
            isum = int(it.sum())
            if isum != 32768:
                fired.append(i * 32 + j)
                diff = isum - 32768
                k = np.unravel_index(np.argmin(fl) if diff > 0 else np.argmax(fl), (2, 2))
                it[k] -= diff
            out[i * 32 + j] = it.reshape(4)
    return out, fired


def weights(frac):
    """N14: the four integer weights of a fraction word"""
    a, b = frac & 31, frac >> 5
    return 32 * (32 - a) * (32 - b), 32 * a * (32 - b), 32 * (32 - a) * b, 32 * a * b


def remap(src, xy, frac, value=0):
    """N14, vectorised; src [sh, sw] or [sh, sw, c] uint8"""
    src = np.asarray(src, np.uint8)
    s3 = src.reshape(src.shape[0], src.shape[1], -1).astype(np.int64)
    sh, sw, c = s3.shape
    x, y = xy[..., 0].astype(np.int64), xy[..., 1].astype(np.int64)
    acc = np.full(x.shape + (c,), 1 << 14, np.int64)
    for (dy, dx), wt in zip(((0, 0), (0, 1), (1, 0), (1, 1)), weights(frac.astype(np.int64))):
        xx, yy = x + dx, y + dy
        inside = (xx >= 0) & (xx < sw) & (yy >= 0) & (yy < sh)
        p = np.where(inside[..., None], s3[np.clip(yy, 0, sh - 1), np.clip(xx, 0, sw - 1)], int(value))
        acc += wt[..., None] * p
    out = (acc >> 15).astype(np.uint8)
    return out if src.ndim == 3 else out[..., 0]


def remap_loop(src, xy, frac, value=0):
    """N14 pixel by pixel, as the sentence reads"""
    src = np.asarray(src, np.uint8)
    s3 = src.reshape(src.shape[0], src.shape[1], -1)
    sh, sw, c = s3.shape
    h, w = frac.shape
    out = np.zeros((h, w, c), np.uint8)
    for i in range(h):
        for j in range(w):
            a, b = int(frac[i, j]) & 31, int(frac[i, j]) >> 5
            wt = (32 * (32 - a) * (32 - b), 32 * a * (32 - b), 32 * (32 - a) * b, 32 * a * b)
            for ch in range(c):
                s = 1 << 14
                for t, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
                    xx, yy = int(xy[i, j, 0]) + dx, int(xy[i, j, 1]) + dy
                    s += wt[t] * (int(s3[yy, xx, ch]) if 0 <= xx < sw and 0 <= yy < sh else int(value))
                out[i, j, ch] = s >> 15
    return out if src.ndim == 3 else out[..., 0]


def taps_outside(xy, src_size):
    """how many of a pixel's four taps lie outside a source of (sw, sh) -> int [h, w]"""
    sw, sh = src_size
    x, y = xy[..., 0].astype(np.int64), xy[..., 1].astype(np.int64)
    n = np.zeros(x.shape, np.int64)
    for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
        n += ~((x + dx >= 0) & (x + dx < sw) & (y + dy >= 0) & (y + dy < sh))
    return n
