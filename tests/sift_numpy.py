"""numpy restatement of the SIFT extractor (ros_stereo_slam_amd/csrc/sift.hip): detection and descriptors of OpenCV 3.2's
xfeatures2d::SIFT as recalled, stated operation by operation so that the device code can be held to it bit for bit.  OpenCV
is not available here: every point below marked S<k> is "upstream, from memory -- verify" (DESIGN.md section 10d lists
them); the points marked OURS are choices this project makes where upstream leaves the result open.

All image arithmetic is IEEE float32, one rounding per written operation (no fused multiply-add), evaluated left to right as
written; sqrt and / are the correctly rounded ones.  Kernel coefficients, layer sigmas and the exp / cos / sin arguments go
through float64 where stated.

OURS-1  exp is svo_exp, cos / sin are svo_cos / svo_sin of include/svo_math.h (ported below, double operation for double
        operation); expf(x) := (float)svo_exp((double)x), cosf / sinf alike; powf(2, t) := (float)svo_exp((double)t * LN2);
        2^(1/n) := svo_exp(LN2 / n) and its powers are running products.
OURS-2  separable blur: row pass over the whole image, then column pass over its result; each pass is
        acc = k[0] * p[0]; acc = acc + k[i] * p[i] for i = 1 .. ksize - 1 (taps in index order).
OURS-3  histogram sums (orientation and descriptor) are order-free: every contribution v (float32) enters as the integer
        rint((double)v * 2^20), the integers are added exactly (int64), the bin is (float)((double)sum * 2^-20).
OURS-4  output order: ascending (octave, layer, row, column) of the REFINED extremum, then ascending orientation bin.
        Duplicates (several starting pixels whose refinement ends in the same cell -- they carry identical fields, which is
        upstream's removeDuplicated criterion) are one key point.
"""
import math

import numpy as np

f32, f64 = np.float32, np.float64
LN2 = 0.6931471805599453
IMG_BORDER, MAX_INTERP_STEPS, ORI_BINS = 5, 5, 36
Q_SCALE, Q_INV = 1048576.0, 1.0 / 1048576.0


# ---- include/svo_math.h, ported ----
def svo_exp(x):
    x = np.asarray(x, f64)
    LN2_HI, LN2_LO, INV_LN2 = 6.93147180369123816490e-01, 1.90821492927058770002e-10, 1.44269504088896338700e+00
    P1, P2, P3 = 1.66666666666666019037e-01, -2.77777777770155933842e-03, 6.61375632143793436117e-05
    P4, P5 = -1.65339022054652515390e-06, 4.13813679705723846039e-08
    xc = np.clip(x, -708.0, 709.0)
    k = np.rint(xc * INV_LN2)
    hi = xc - k * LN2_HI
    lo = k * LN2_LO
    r = hi - lo
    t = r * r
    c = r - t * (P1 + t * (P2 + t * (P3 + t * (P4 + t * P5))))
    y = 1.0 - ((lo - (r * c) / (2.0 - c)) - hi)
    y = np.atleast_1d(y)
    out = (y.view(np.int64) + (np.atleast_1d(k).astype(np.int64) << 52)).view(f64).reshape(x.shape)
    out = np.where(x > 709.0, np.inf, np.where(x < -708.0, 0.0, out))
    return out if out.ndim else f64(out)


def _ksin(x):
    S1, S2, S3 = -1.66666666666666324348e-01, 8.33333333332248946124e-03, -1.98412698298579493134e-04
    S4, S5, S6 = 2.75573137070700676789e-06, -2.50507602534068634195e-08, 1.58969099521155010221e-10
    z = x * x
    r = S2 + z * (S3 + z * (S4 + z * (S5 + z * S6)))
    return x + (z * x) * (S1 + z * r)


def _kcos(x):
    C1, C2, C3 = 4.16666666666666019037e-02, -1.38888888888741095749e-03, 2.48015872894767294178e-05
    C4, C5, C6 = -2.75573143513906633035e-07, 2.08757232129817482790e-09, -1.13596475577881948265e-11
    z = x * x
    r = z * (C1 + z * (C2 + z * (C3 + z * (C4 + z * (C5 + z * C6)))))
    hz = 0.5 * z
    w = 1.0 - hz
    return w + (((1.0 - w) - hz) + z * r)


def _reduce(x):
    k = np.rint(x * 6.36619772367581382433e-01)
    r = x - k * 1.57079632673412561417e+00
    r = r - k * 6.07710050630396597660e-11
    r = r - k * 2.02226624871116645580e-21
    r = r - k * 8.47842766036889956997e-32
    return r, k.astype(np.int64) & 3


def svo_sin(x):
    r, q = _reduce(np.asarray(x, f64))
    s, c = _ksin(r), _kcos(r)
    return np.where(q == 0, s, np.where(q == 1, c, np.where(q == 2, -s, -c)))


def svo_cos(x):
    r, q = _reduce(np.asarray(x, f64))
    s, c = _ksin(r), _kcos(r)
    return np.where(q == 0, c, np.where(q == 1, -s, np.where(q == 2, -c, s)))


def expf(x):
    return svo_exp(np.asarray(x, f32).astype(f64)).astype(f32)


def fast_atan2(y, x):
    """S20: cv::fastAtan2, degrees in [0, 360) (orb_cv.hip states the same polynomial)"""
    y, x = np.asarray(y, f32), np.asarray(x, f32)
    k = f32(180 / 3.14159265358979323846)
    p1, p3, p5, p7 = (f32(0.9997878412794807) * k, f32(-0.3258083974640975) * k, f32(0.1555786518463281) * k,
                      f32(-0.04432655554792128) * k)
    eps = f32(2.2204460492503131e-16)
    ax, ay = np.abs(x), np.abs(y)
    big = ax >= ay
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.where(big, ay / (ax + eps), ax / (ay + eps)).astype(f32)
    c2 = c * c
    a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c
    a = np.where(big, a, f32(90) - a)
    a = np.where(x < 0, f32(180) - a, a)
    a = np.where(y < 0, f32(360) - a, a)
    return a.astype(f32)


def cv_round(v):
    return int(np.rint(v))


# ---- scale space ----
def gray_u8(img):
    """S1: cvtColor BGR2GRAY on 8-bit: (1868 B + 9617 G + 4899 R + 8192) >> 14"""
    img = np.asarray(img, np.uint8)
    if img.ndim == 2:
        return img
    if img.shape[2] == 1:
        return img[:, :, 0]
    b, g, r = (img[:, :, k].astype(np.int32) for k in range(3))
    return ((1868 * b + 9617 * g + 4899 * r + 8192) >> 14).astype(np.uint8)


def _linear_tab(n):
    """S2: cv::resize INTER_LINEAR to 2n: fx = (dx + 0.5) * 0.5 - 0.5, sx = floor(fx), fx -= sx; sx < 0 -> (0, 0);
    sx >= n - 1 -> (n - 1, 0); the taps are S[sx] * (1 - fx) + S[min(sx + 1, n - 1)] * fx"""
    d = np.arange(2 * n)
    fx = ((d + 0.5) * 0.5 - 0.5).astype(f32)
    sx = np.floor(fx).astype(np.int64)
    fx = (fx - sx.astype(f32)).astype(f32)
    lo = sx < 0
    sx[lo], fx[lo] = 0, 0
    hi = sx >= n - 1
    sx[hi], fx[hi] = n - 1, 0
    return sx, np.minimum(sx + 1, n - 1), (f32(1) - fx).astype(f32), fx


def upsample2(g):
    """horizontal pass, then vertical pass, float32"""
    h, w = g.shape
    x0, x1, a0, a1 = _linear_tab(w)
    y0, y1, b0, b1 = _linear_tab(h)
    t = g[:, x0] * a0[None, :] + g[:, x1] * a1[None, :]
    return (t[y0, :] * b0[:, None] + t[y1, :] * b1[:, None]).astype(f32)


def gauss_kernel(sigma):
    """S5 / S6: ksize = cvRound(sigma * 8 + 1) | 1; t_i = exp(-0.5 / sigma^2 * x * x), x = i - (ksize - 1) / 2, in double;
    cf_i = (float)t_i; sum (double) of the cf_i in index order; cf_i = (float)(cf_i * (1 / sum))"""
    sigma = float(sigma)
    n = cv_round(sigma * 8 + 1) | 1
    s2x = -0.5 / (sigma * sigma)
    x = np.arange(n, dtype=f64) - (n - 1) * 0.5
    cf = svo_exp(s2x * x * x).astype(f32)
    s = 0.0
    for v in cf:
        s += float(v)
    s = 1.0 / s
    return (cf.astype(f64) * s).astype(f32)


def reflect101(p, n):
    """S7: cv::borderInterpolate, BORDER_REFLECT_101 (repeated until inside; a length of 1 gives 0)"""
    p = np.asarray(p, np.int64).copy()
    if n == 1:
        return np.zeros_like(p)
    while True:
        lo, hi = p < 0, p >= n
        if not (lo.any() or hi.any()):
            return p
        p[lo] = -p[lo]
        p[hi] = 2 * (n - 1) - p[hi]


def blur(img, k):
    """OURS-2"""
    h, w = img.shape
    r = len(k) // 2
    cols = [reflect101(np.arange(w) + t - r, w) for t in range(len(k))]
    acc = k[0] * img[:, cols[0]]
    for t in range(1, len(k)):
        acc = acc + k[t] * img[:, cols[t]]
    rows = [reflect101(np.arange(h) + t - r, h) for t in range(len(k))]
    out = k[0] * acc[rows[0], :]
    for t in range(1, len(k)):
        out = out + k[t] * acc[rows[t], :]
    return out.astype(f32)


def layer_sigmas(sigma, n):
    """S4: sig[0] = sigma; sig[i] = sqrt(total^2 - prev^2), prev = k^(i-1) sigma, total = prev k, k = 2^(1/n), in double"""
    k = float(svo_exp(LN2 / n))
    sig, p = [float(sigma)], 1.0
    for _ in range(1, n + 3):
        prev = p * sigma
        total = prev * k
        sig.append(math.sqrt(total * total - prev * prev))
        p = p * k
    return sig


def n_octaves(w, h):
    """S3: cvRound(log2(min(w2, h2)) - 2) + 1 on the doubled size (never a tie: log2 of an integer is not k + 1/2)"""
    return cv_round(math.log(float(min(2 * w, 2 * h))) / math.log(2.0) - 2) + 1


def build_pyramid(img, n=3, sigma=1.6):
    """-> (gauss, dog): lists per octave of float32 arrays [n + 3, h, w] and [n + 2, h, w]"""
    g = gray_u8(img).astype(f32)
    base = upsample2(g)
    sf = f32(sigma)
    sig_diff = np.sqrt(np.maximum(sf * sf - f32(0.5) * f32(0.5) * f32(4), f32(0.01)))   # S2, float
    base = blur(base, gauss_kernel(float(sig_diff)))
    sig = layer_sigmas(float(sigma), n)
    kern = [None] + [gauss_kernel(s) for s in sig[1:]]
    gauss, dog = [], []
    for o in range(n_octaves(g.shape[1], g.shape[0])):
        if o > 0:
            prev = gauss[o - 1][n]
            base = prev[0:2 * (prev.shape[0] // 2):2, 0:2 * (prev.shape[1] // 2):2]   # S4: INTER_NEAREST to (w / 2, h / 2)
        lay = [np.ascontiguousarray(base, f32)]
        for i in range(1, n + 3):
            lay.append(blur(lay[i - 1], kern[i]))
        G = np.stack(lay)
        gauss.append(G)
        dog.append((G[1:] - G[:-1]).astype(f32))   # S8
    return gauss, dog


# ---- extrema and refinement ----
def _derivs(D, l, r, c):
    """S10: the finite differences of adjustLocalExtrema at (layer, row, column) arrays"""
    img_scale = f32(1) / f32(255)
    ds, ss, cs = img_scale * f32(0.5), img_scale, img_scale * f32(0.25)
    v = D[l, r, c]
    dD = ((D[l, r, c + 1] - D[l, r, c - 1]) * ds, (D[l, r + 1, c] - D[l, r - 1, c]) * ds, (D[l + 1, r, c] - D[l - 1, r, c]) * ds)
    v2 = v * f32(2)
    dxx = (D[l, r, c + 1] + D[l, r, c - 1] - v2) * ss
    dyy = (D[l, r + 1, c] + D[l, r - 1, c] - v2) * ss
    dss = (D[l + 1, r, c] + D[l - 1, r, c] - v2) * ss
    dxy = (D[l, r + 1, c + 1] - D[l, r + 1, c - 1] - D[l, r - 1, c + 1] + D[l, r - 1, c - 1]) * cs
    dxs = (D[l + 1, r, c + 1] - D[l + 1, r, c - 1] - D[l - 1, r, c + 1] + D[l - 1, r, c - 1]) * cs
    dys = (D[l + 1, r + 1, c] - D[l + 1, r - 1, c] - D[l - 1, r + 1, c] + D[l - 1, r - 1, c]) * cs
    return v, dD, (dxx, dyy, dss, dxy, dxs, dys)


def _solve3(H, b):
    """S11: Matx33f::solve(DECOMP_LU) = Cramer's rule in float; a zero determinant gives the zero vector"""
    dxx, dyy, dss, dxy, dxs, dys = H
    a00, a01, a02, a10, a11, a12, a20, a21, a22 = dxx, dxy, dxs, dxy, dyy, dys, dxs, dys, dss
    b0, b1, b2 = b
    det = a00 * (a11 * a22 - a12 * a21) - a01 * (a10 * a22 - a12 * a20) + a02 * (a10 * a21 - a11 * a20)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = f32(1) / det
        x0 = d * (b0 * (a11 * a22 - a12 * a21) - a01 * (b1 * a22 - a12 * b2) + a02 * (b1 * a21 - a11 * b2))
        x1 = d * (a00 * (b1 * a22 - a12 * b2) - b0 * (a10 * a22 - a12 * a20) + a02 * (a10 * b2 - b1 * a20))
        x2 = d * (a00 * (a11 * b2 - b1 * a21) - a01 * (a10 * b2 - b1 * a20) + b0 * (a10 * a21 - a11 * a20))
    z = det == 0
    return np.where(z, f32(0), x0).astype(f32), np.where(z, f32(0), x1).astype(f32), np.where(z, f32(0), x2).astype(f32)


def find_cells(D, n, contrast_threshold, edge_threshold):
    """S9 - S13 on one octave's DoG stack D [n + 2, h, w] -> sorted unique refined cells (layer, row, col) and their
    (xi, xr, xc, contr)"""
    L, h, w = D.shape
    thr = math.floor(0.5 * contrast_threshold / n * 255)
    B = IMG_BORDER
    empty = (np.zeros(0, np.int64),) * 3 + (np.zeros(0, f32),) * 4
    if h <= 2 * B or w <= 2 * B:
        return empty
    ls, rs, cs = [], [], []
    for i in range(1, n + 1):
        val = D[i, B:h - B, B:w - B]
        mx = np.full(val.shape, -np.inf, f32)
        mn = np.full(val.shape, np.inf, f32)
        for dl in (-1, 0, 1):
            for dr in (-1, 0, 1):
                for dc in (-1, 0, 1):
                    nb = D[i + dl, B + dr:h - B + dr, B + dc:w - B + dc]
                    mx = np.maximum(mx, nb)
                    mn = np.minimum(mn, nb)
        cand = (np.abs(val) > f32(thr)) & (((val > 0) & (val >= mx)) | ((val < 0) & (val <= mn)))   # S9
        r, c = np.nonzero(cand)
        ls.append(np.full(len(r), i, np.int64))
        rs.append(r + B)
        cs.append(c + B)
    l, r, c = np.concatenate(ls), np.concatenate(rs), np.concatenate(cs)
    N = len(l)
    if N == 0:
        return empty
    state = np.zeros(N, np.int8)   # 0 iterating, 1 converged, -1 rejected
    xi, xr, xc = np.zeros(N, f32), np.zeros(N, f32), np.zeros(N, f32)
    big = f32(2147483647 // 3)
    for _ in range(MAX_INTERP_STEPS):   # S10
        a = np.flatnonzero(state == 0)
        if len(a) == 0:
            break
        _, dD, H = _derivs(D, l[a], r[a], c[a])
        X0, X1, X2 = _solve3(H, dD)
        txi, txr, txc = -X2, -X1, -X0
        xi[a], xr[a], xc[a] = txi, txr, txc
        conv = (np.abs(txi) < f32(0.5)) & (np.abs(txr) < f32(0.5)) & (np.abs(txc) < f32(0.5))
        state[a[conv]] = 1
        mv = ~conv
        huge = mv & ~((np.abs(txi) <= big) & (np.abs(txr) <= big) & (np.abs(txc) <= big))   # also catches NaN
        state[a[huge]] = -1
        mv &= ~huge
        am = a[mv]
        c[am] += np.rint(txc[mv]).astype(np.int64)
        r[am] += np.rint(txr[mv]).astype(np.int64)
        l[am] += np.rint(txi[mv]).astype(np.int64)
        out = (l[am] < 1) | (l[am] > n) | (c[am] < B) | (c[am] >= w - B) | (r[am] < B) | (r[am] >= h - B)
        state[am[out]] = -1
    keep = np.flatnonzero(state == 1)   # still iterating after 5 steps: rejected
    l, r, c, xi, xr, xc = l[keep], r[keep], c[keep], xi[keep], xr[keep], xc[keep]
    v, dD, H = _derivs(D, l, r, c)
    t = dD[0] * xc + dD[1] * xr + dD[2] * xi
    contr = v * (f32(1) / f32(255)) + t * f32(0.5)
    ok = ~(np.abs(contr) * f32(n) < f32(contrast_threshold))   # S12
    dxx, dyy, _, dxy, _, _ = H
    tr = dxx + dyy
    det = dxx * dyy - dxy * dxy
    et = f32(edge_threshold)
    ok &= ~((det <= 0) | (tr * tr * et >= (et + f32(1)) * (et + f32(1)) * det))   # S13
    l, r, c, xi, xr, xc, contr = (a[ok] for a in (l, r, c, xi, xr, xc, contr))
    key = (l * h + r) * w + c
    _, first = np.unique(key, return_index=True)   # OURS-4: sorted by (layer, row, col), one per cell
    return tuple(a[first] for a in (l, r, c, xi, xr, xc, contr))


def _quant_sum(bins, v, size):
    """OURS-3"""
    q = np.rint(np.asarray(v, f32).astype(f64) * Q_SCALE).astype(np.int64)
    acc = np.zeros(size, np.int64)
    np.add.at(acc, bins, q)
    return (acc.astype(f64) * Q_INV).astype(f32)


def orientation_hist(img, px, py, radius, sigma):
    """S15 / S16: calcOrientationHist -> the smoothed 36-bin histogram"""
    n = ORI_BINS
    h, w = img.shape
    expf_scale = f32(-1) / (f32(2) * sigma * sigma)
    o = np.arange(-radius, radius + 1)
    ys, xs = py + o, px + o
    oi, oj = o[(ys > 0) & (ys < h - 1)], o[(xs > 0) & (xs < w - 1)]
    I, J = np.meshgrid(oi, oj, indexing="ij")
    I, J = I.ravel(), J.ravel()
    y, x = py + I, px + J
    dx = img[y, x + 1] - img[y, x - 1]
    dy = img[y - 1, x] - img[y + 1, x]
    W = expf((I * I + J * J).astype(f32) * expf_scale)
    ori = fast_atan2(dy, dx)
    mag = np.sqrt(dx * dx + dy * dy)
    b = np.rint((f32(n) / f32(360)) * ori).astype(np.int64)
    b = np.where(b >= n, b - n, b)
    b = np.where(b < 0, b + n, b)
    t = _quant_sum(b, W * mag, n)
    tm2, tm1, tp1, tp2 = np.roll(t, 2), np.roll(t, 1), np.roll(t, -1), np.roll(t, -2)
    return (tm2 + tp2) * (f32(1) / f32(16)) + (tm1 + tp1) * (f32(4) / f32(16)) + t * (f32(6) / f32(16))


def orientation_peaks(hist):
    """S17: -> [(bin index, angle)] in ascending bin order"""
    n = ORI_BINS
    thr = hist.max() * f32(0.8)
    out = []
    for j in range(n):
        hl, hj, hr = hist[(j - 1) % n], hist[j], hist[(j + 1) % n]
        if hj > hl and hj > hr and hj >= thr:
            b = f32(j) + f32(0.5) * (hl - hr) / (hl - f32(2) * hj + hr)
            b = f32(n) + b if b < 0 else (b - f32(n) if b >= n else b)
            ang = f32(360) - (f32(360) / f32(n)) * b
            if abs(ang - f32(360)) < f32(1.1920929e-07):
                ang = f32(0)
            out.append((j, f32(ang)))
    return out


def unpack_octave(octave):
    """S19"""
    o, layer = octave & 255, (octave >> 8) & 255
    o = o if o < 128 else (-128 | o)
    scale = f32(1) / f32(1 << o) if o >= 0 else f32(1 << -o)
    return o, layer, scale


def raw_descriptor(img, ptx, pty, ori, scl):
    """S19: calcSIFTDescriptor up to the 128 histogram values (before normalisation)"""
    d, n = 4, 8
    h, w = img.shape
    px, py = cv_round(ptx), cv_round(pty)
    a = ori * f32(math.pi / 180)
    cos_t, sin_t = f32(svo_cos(f64(a))), f32(svo_sin(f64(a)))
    bins_per_rad = f32(n) / f32(360)
    exp_scale = f32(-1) / (f32(d * d) * f32(0.5))
    hist_width = f32(3) * scl
    radius = cv_round(hist_width * f32(1.4142135623730951) * f32(d + 1) * f32(0.5))
    radius = min(radius, int(math.sqrt(float(w) * w + float(h) * h)))
    cos_t, sin_t = cos_t / hist_width, sin_t / hist_width
    o = np.arange(-radius, radius + 1)
    ys, xs = py + o, px + o
    oi, oj = o[(ys > 0) & (ys < h - 1)], o[(xs > 0) & (xs < w - 1)]
    I, J = np.meshgrid(oi, oj, indexing="ij")
    I, J = I.ravel(), J.ravel()
    fi, fj = I.astype(f32), J.astype(f32)
    c_rot = fj * cos_t - fi * sin_t
    r_rot = fj * sin_t + fi * cos_t
    rbin = r_rot + f32(d // 2) - f32(0.5)
    cbin = c_rot + f32(d // 2) - f32(0.5)
    m = (rbin > -1) & (rbin < d) & (cbin > -1) & (cbin < d)
    I, J, c_rot, r_rot, rbin, cbin = (v[m] for v in (I, J, c_rot, r_rot, rbin, cbin))
    y, x = py + I, px + J
    dx = img[y, x + 1] - img[y, x - 1]
    dy = img[y - 1, x] - img[y + 1, x]
    W = expf((c_rot * c_rot + r_rot * r_rot) * exp_scale)
    obin = (fast_atan2(dy, dx) - ori) * bins_per_rad
    mag = np.sqrt(dx * dx + dy * dy) * W
    r0, c0, o0 = np.floor(rbin), np.floor(cbin), np.floor(obin)
    rbin, cbin, obin = rbin - r0, cbin - c0, obin - o0
    r0, c0, o0 = r0.astype(np.int64), c0.astype(np.int64), o0.astype(np.int64)
    o0 = np.where(o0 < 0, o0 + n, o0)
    o0 = np.where(o0 >= n, o0 - n, o0)
    v_r1 = mag * rbin
    v_r0 = mag - v_r1
    v_rc11 = v_r1 * cbin
    v_rc10 = v_r1 - v_rc11
    v_rc01 = v_r0 * cbin
    v_rc00 = v_r0 - v_rc01
    v111 = v_rc11 * obin
    v110 = v_rc11 - v111
    v101 = v_rc10 * obin
    v100 = v_rc10 - v101
    v011 = v_rc01 * obin
    v010 = v_rc01 - v011
    v001 = v_rc00 * obin
    v000 = v_rc00 - v001
    idx = ((r0 + 1) * (d + 2) + c0 + 1) * (n + 2) + o0
    S, T = n + 2, (d + 2) * (n + 2)
    bins = np.concatenate([idx, idx + 1, idx + S, idx + S + 1, idx + T, idx + T + 1, idx + T + S, idx + T + S + 1])
    vals = np.concatenate([v000, v001, v010, v011, v100, v101, v110, v111])
    hist = _quant_sum(bins, vals, (d + 2) * (d + 2) * (n + 2)).reshape(d + 2, d + 2, n + 2)
    hist[:, :, 0] = hist[:, :, 0] + hist[:, :, n]
    hist[:, :, 1] = hist[:, :, 1] + hist[:, :, n + 1]
    return hist[1:d + 1, 1:d + 1, :n].reshape(d * d * n).copy()


def finish_descriptors(raw):
    """S19: normalise, clip at 0.2, renormalise x 512, saturate_cast<uchar>; the two sums of 128 squares run in index order"""
    raw = np.asarray(raw, f32).reshape(-1, 128)
    nrm2 = np.zeros(len(raw), f32)
    for k in range(128):
        nrm2 = nrm2 + raw[:, k] * raw[:, k]
    thr = np.sqrt(nrm2) * f32(0.2)
    val = np.minimum(raw, thr[:, None])
    nrm2 = np.zeros(len(raw), f32)
    for k in range(128):
        nrm2 = nrm2 + val[:, k] * val[:, k]
    s = f32(512) / np.maximum(np.sqrt(nrm2), f32(1.1920929e-07))
    return np.clip(np.rint(val * s[:, None]), 0, 255).astype(f32)


def describe(gauss, xy, size, angle, octave, n=3):
    """detector->compute on public key points (S19) against a pyramid of build_pyramid"""
    raw = np.zeros((len(xy), 128), f32)
    for i in range(len(xy)):
        o, layer, scale = unpack_octave(int(octave[i]))
        img = gauss[o + 1][layer]
        ang = f32(360) - f32(angle[i])
        if abs(ang - f32(360)) < f32(1.1920929e-07):
            ang = f32(0)
        raw[i] = raw_descriptor(img, f32(xy[i, 0]) * scale, f32(xy[i, 1]) * scale, ang, f32(size[i]) * scale * f32(0.5))
    return finish_descriptors(raw)


def sift(img, n_features=0, n_octave_layers=3, contrast_threshold=0.04, edge_threshold=10.0, sigma=1.6, descriptors=True,
         pyramid=None):
    """-> dict(xy [n, 2], size, angle, response (float32), octave (int32, cv's packed field), desc [n, 128] float32 or None,
    gauss, dog)"""
    n = n_octave_layers
    gauss, dog = pyramid if pyramid is not None else build_pyramid(img, n, sigma)
    sf = f32(sigma)
    X, Y, S, A, R, O = [], [], [], [], [], []
    for o, D in enumerate(dog):
        l, r, c, xi, xr, xc, contr = find_cells(D, n, contrast_threshold, edge_threshold)
        if len(l) == 0:
            continue
        po = f32(1 << o)
        ptx = (c.astype(f32) + xc) * po   # S14
        pty = (r.astype(f32) + xr) * po
        packed = o + (l << 8) + (np.rint((xi.astype(f64) + 0.5) * 255).astype(np.int64) << 16)
        size = sf * svo_exp(((l.astype(f32) + xi) / f32(n)).astype(f64) * LN2).astype(f32) * po * f32(2)
        resp = np.abs(contr)
        scl = size * f32(0.5) / po
        for i in range(len(l)):
            hist = orientation_hist(gauss[o][l[i]], int(c[i]), int(r[i]), cv_round(f32(4.5) * scl[i]), f32(1.5) * scl[i])
            for _, ang in orientation_peaks(hist):
                X.append(ptx[i]); Y.append(pty[i]); S.append(size[i]); A.append(ang); R.append(resp[i]); O.append(packed[i])
    xy = np.stack([np.array(X, f32), np.array(Y, f32)], axis=1) if X else np.zeros((0, 2), f32)
    size, angle, resp, octv = np.array(S, f32), np.array(A, f32), np.array(R, f32), np.array(O, np.int64)
    if n_features > 0 and len(resp) > n_features:   # S18: retainBest, ties kept
        nth = np.sort(resp)[::-1][n_features - 1]
        k = resp >= nth
        xy, size, angle, resp, octv = xy[k], size[k], angle[k], resp[k], octv[k]
    # S18: the doubled first octave: octave - 1 in the low byte, pt and size halved
    octv = ((octv & ~255) | ((octv - 1) & 255)).astype(np.int32)
    xy, size = xy * f32(0.5), size * f32(0.5)
    desc = describe(gauss, xy, size, angle, octv, n) if descriptors else None
    return dict(xy=xy, size=size, angle=angle, response=resp, octave=octv, desc=desc, gauss=gauss, dog=dog)
