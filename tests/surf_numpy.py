"""numpy restatement of the SURF extractor (ros_stereo_slam_amd/csrc/surf.hip): detect and compute of OpenCV 3.2's
xfeatures2d::SURF as recalled, stated operation by operation so that the device code can be held to it bit for bit
(tests/test_gpu_surf.py).  OpenCV is not available here: every point marked U<k> is "upstream, from memory -- verify"
(DESIGN.md section 10f lists them, and where they differ from the recollection the feature was specified with); the points
marked OURS are choices this project makes where upstream leaves the result open.

All arithmetic is IEEE float32 / float64 as written, one rounding per written operation (no fused multiply-add), evaluated
left to right; / and sqrt are the correctly rounded ones; cvRound is round-half-to-even.

U1   SURF::create(hessianThreshold = 100, nOctaves = 4, nOctaveLayers = 3, extended = false, upright = false);
     SURF_HAAR_SIZE0 9, SURF_HAAR_SIZE_INC 6, SURF_ORI_SEARCH_INC 5, SURF_ORI_SIGMA 2.5f, SURF_DESC_SIGMA 3.3f, ORI_RADIUS 6,
     ORI_WIN 60, PATCH_SZ 20.
U2   BGR -> grey by cvtColor's integer weights; integral(grey, CV_32S): (h + 1) x (w + 1), zero first row and column.
U3   octave o, layer l in 0 ... nOctaveLayers + 1: size (9 + 6 l) << o, step 1 << o, planes of (h / step) x (w / step) floats
     that start at zero; a layer whose size exceeds w or h stays zero.
U4   resizeHaarPattern: ratio = (float)new / old, corners cvRound(ratio * src), w = src[4] / ((float)(dx2 - dx1) * (dy2 - dy1)).
U5   calcHaarPattern: d (double) += (float)(int box sum) * w, the product in float; result (float)d.  det = dx * dy -
     0.81f * dxy * dxy, trace = dx + dy at (i + margin, j + margin), margin = (size / 2) / step, 1 + (h - size) / step sample
     rows and 1 + (w - size) / step columns.
U6   maxima of layers 1 ... nOctaveLayers: margin = (sizes[l + 1] / 2) / step + 1, val > (float)threshold and val > each of the
     26 neighbours; centre = step * (i - (size / 2) / step) + (size - 1) * 0.5f; class_id = sign of the trace.
U7   interpolateKeypoint: central differences, x = A.solve(b, DECOMP_LU) on a Matx33f -- recalled as Matx_FastSolveOp<float, 3, 1>,
     CRAMER'S RULE in float with d = 1 / det (not an LU elimination: here this restatement differs from the recollection the
     feature was specified with); a zero determinant gives x = 0.  Accepted when x != 0 and every |x_k| <= 1; pt += x * step,
     size = (float)cvRound(size + x2 * (sizes[l] - sizes[l - 1])).
U8   the list is sorted by KeypointGreater: response descending, then size descending, octave descending, pt.y descending,
     pt.x ascending.
OURS-1  the remaining ties are broken by ascending (octave, layer, row, column) of the sample: a total order, so the device's
     append order can never show.
U9   s = size * 1.2f / 9.0f, grad_wav_size = 2 * cvRound(2 * s); dropped when the integral image has fewer rows or columns
     than grad_wav_size; samples (i, j), i outer, j inner, with i^2 + j^2 <= 36 -- 113 of them (the 109 of the specification
     is the count of i^2 + j^2 < 36); weights G[i + 6] * G[j + 6], G = getGaussianKernel(13, 2.5, CV_32F): c_k =
     (float)exp(-0.5 / sigma^2 * x * x), x = k - 6, sum (double) of the floats in index order, c_k = (float)(c_k * (1 / sum)),
     exp = svo_exp.  Position cvRound(c + a * s - (float)(grad_wav_size - 1) / 2); a sample with x or y outside
     0 ... (w + 1 or h + 1) - grad_wav_size - 1 is skipped, a key point with none is dropped.  X = dx * weight, Y = dy * weight,
     angle = fastAtan2(Y, X); for i = 0, 5 ... 355 the X and Y with d = |cvRound(angle) - i| < 30 or > 330 are added IN SAMPLE
     ORDER in float (upstream's own sequential order: nothing is left open, so no fixed-point sums are needed); the first
     window with the largest sumx^2 + sumy^2 > 0 wins; kp.angle = fastAtan2(-besty, bestx).
U10  win_size = (int)(21 * s).  Rotated window: rad = angle * (float)(pi / 180), sin_dir = -(float)svo_sin(rad), cos_dir =
     (float)svo_cos(rad); start = centre +- win_offset terms in float, one float addition per row, one DOUBLE addition per
     column (both sequential, as upstream's loops); bilinear in float from the grey image, cvRound; outside (ix or iy not in
     0 ... size - 2): the pixel at the clamped cvRound position.  upright: angle 270, the window unrotated (upstream's
     transposed indexing kept).  resize to 21 x 21, INTER_AREA, see OURS-2.  DX / DY over 2 x 2 times the 20 x 20 Gaussian
     weights (sigma 3.3), 4 x 4 cells of 5 x 5 summed in row-major order in float, square_mag in double cell after cell,
     scale = (float)(1 / (sqrt(square_mag) + FLT_EPSILON)).
OURS-2  INTER_AREA as cv::resize is recalled: scale = 1 / (21.0 / win_size); when |scale - cvRound(scale)| < DBL_EPSILON the
     integer path (k x k integer sums; k = 2: (sum + 2) >> 2; else cvRound((float)sum * (1.f / (k * k)))); otherwise
     computeResizeAreaTab's weights (left fraction, whole cells at 1 / cellWidth, right fraction, thresholds 1e-3, as floats),
     buf[dx] = 0 + S * alpha over the table in ascending source column, sum[dy] = 0 + beta * buf over ascending source row,
     saturate_cast<uchar>(sum).  This is upstream's serial order; it is fixed here because the device spreads rows over lanes.
OURS-3  compute() on key points from elsewhere: a position that is not finite or beyond +-65536, or a size whose window
     (int)(21 s) is not in 21 ... 65536 (upstream would enlarge a smaller window by another interpolation), is dropped like a
     key point whose wavelet does not fit.  The detector yields no such key point (size >= 9 gives a window of 25).
"""
import numpy as np

from brief_numpy import integral, to_grey
from sift_numpy import fast_atan2, svo_cos, svo_exp, svo_sin

f32, f64 = np.float32, np.float64
HAAR_SIZE0, HAAR_SIZE_INC, ORI_SEARCH_INC, ORI_SIGMA, DESC_SIGMA = 9, 6, 5, 2.5, 3.3
ORI_RADIUS, ORI_WIN, PATCH_SZ = 6, 60, 20
FLT_EPSILON, DBL_EPSILON = f32(1.1920928955078125e-07), 2.220446049250313e-16

DX_S = ((0, 2, 3, 7, 1), (3, 2, 6, 7, -2), (6, 2, 9, 7, 1))
DY_S = ((2, 0, 7, 3, 1), (2, 3, 7, 6, -2), (2, 6, 7, 9, 1))
DXY_S = ((1, 1, 4, 4, 1), (5, 1, 8, 4, -1), (1, 5, 4, 8, -1), (5, 5, 8, 8, 1))
GDX_S = ((0, 0, 2, 4, -1), (2, 0, 4, 4, 1))
GDY_S = ((0, 0, 4, 2, 1), (0, 2, 4, 4, -1))


def default_params(**kw):
    p = dict(hessian_threshold=100.0, n_octaves=4, n_octave_layers=3, extended=0, upright=0)
    p.update(kw)
    return p


def layers_layout(w, h, n_octaves=4, n_octave_layers=3):
    """U3 -> (sizes, steps, lw, lh), one entry per layer, octave after octave"""
    sizes, steps, lw, lh = [], [], [], []
    for o in range(n_octaves):
        for l in range(n_octave_layers + 2):
            sizes.append((HAAR_SIZE0 + HAAR_SIZE_INC * l) << o)
            steps.append(1 << o)
            lw.append(w // (1 << o))
            lh.append(h // (1 << o))
    return sizes, steps, lw, lh


def resize_haar(src, old, new):
    """U4 -> rows (dx1, dy1, dx2, dy2, w)"""
    ratio = f32(new) / f32(old)
    out = []
    for a in src:
        dx1, dy1, dx2, dy2 = (int(np.rint(ratio * f32(v))) for v in a[:4])
        out.append((dx1, dy1, dx2, dy2, f32(a[4]) / (f32(dx2 - dx1) * f32(dy2 - dy1))))
    return out


def calc_haar(S, ys, xs, pat):
    """U5: the pattern at the origins (ys, xs) (broadcastable integer arrays) of the int64 copy S of the integral image"""
    d = None
    for dx1, dy1, dx2, dy2, wgt in pat:
        box = S[ys + dy1, xs + dx1] + S[ys + dy2, xs + dx2] - S[ys + dy2, xs + dx1] - S[ys + dy1, xs + dx2]
        t = (box.astype(f32) * wgt).astype(f64)
        d = t if d is None else d + t
    return (0.0 + d).astype(f32)


def layers(img, n_octaves=4, n_octave_layers=3):
    """U3, U5 -> (det, trace): lists of float32 planes, one per layer"""
    grey = to_grey(img)
    h, w = grey.shape
    S = integral(grey).astype(np.int64)
    sizes, steps, lw, lh = layers_layout(w, h, n_octaves, n_octave_layers)
    dets, traces = [], []
    for size, step, pw, ph in zip(sizes, steps, lw, lh):
        det, tr = np.zeros((ph, pw), f32), np.zeros((ph, pw), f32)
        if size <= h and size <= w:
            ni, nj, m = 1 + (h - size) // step, 1 + (w - size) // step, (size // 2) // step
            ys, xs = (np.arange(ni) * step)[:, None], (np.arange(nj) * step)[None, :]
            dx = calc_haar(S, ys, xs, resize_haar(DX_S, 9, size))
            dy = calc_haar(S, ys, xs, resize_haar(DY_S, 9, size))
            dxy = calc_haar(S, ys, xs, resize_haar(DXY_S, 9, size))
            det[m:m + ni, m:m + nj] = dx * dy - f32(0.81) * dxy * dxy
            tr[m:m + ni, m:m + nj] = dx + dy
        dets.append(det)
        traces.append(tr)
    return dets, traces


def solve3(A, b):
    """U7: Matx33f::solve(b, DECOMP_LU) as Cramer's rule in float; A: 3 x 3 nested float32, b: 3 float32"""
    a = A
    det = (a[0][0] * (a[1][1] * a[2][2] - a[2][1] * a[1][2]) - a[0][1] * (a[1][0] * a[2][2] - a[2][0] * a[1][2])
           + a[0][2] * (a[1][0] * a[2][1] - a[2][0] * a[1][1]))
    if det == 0:
        return [f32(0), f32(0), f32(0)]
    d = f32(1) / det
    x0 = d * (b[0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (b[1] * a[2][2] - a[1][2] * b[2])
              + a[0][2] * (b[1] * a[2][1] - a[1][1] * b[2]))
    x1 = d * (a[0][0] * (b[1] * a[2][2] - a[1][2] * b[2]) - b[0] * (a[1][0] * a[2][2] - a[1][2] * a[2][0])
              + a[0][2] * (a[1][0] * b[2] - b[1] * a[2][0]))
    x2 = d * (a[0][0] * (a[1][1] * b[2] - b[1] * a[2][1]) - a[0][1] * (a[1][0] * b[2] - b[1] * a[2][0])
              + b[0] * (a[1][0] * a[2][1] - a[1][1] * a[2][0]))
    return [x0, x1, x2]


def interpolate(N9, step, ds, x, y, size):
    """U7 -> (ok, x, y, size); N9: [3][9] float32 (layer below, the layer, layer above; row-major 3 x 3)"""
    two, four = f32(2), f32(4)
    b = [-(N9[1][5] - N9[1][3]) / two, -(N9[1][7] - N9[1][1]) / two, -(N9[2][4] - N9[0][4]) / two]
    axy = (N9[1][8] - N9[1][6] - N9[1][2] + N9[1][0]) / four
    axs = (N9[2][5] - N9[2][3] - N9[0][5] + N9[0][3]) / four
    ays = (N9[2][7] - N9[2][1] - N9[0][7] + N9[0][1]) / four
    A = [[N9[1][3] - two * N9[1][4] + N9[1][5], axy, axs],
         [axy, N9[1][1] - two * N9[1][4] + N9[1][7], ays],
         [axs, ays, N9[0][4] - two * N9[1][4] + N9[2][4]]]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        v = solve3(A, b)
        ok = (v[0] != 0 or v[1] != 0 or v[2] != 0) and abs(v[0]) <= 1 and abs(v[1]) <= 1 and abs(v[2]) <= 1
        if not ok:
            return False, x, y, size
        return True, x + v[0] * f32(step), y + v[1] * f32(step), f32(np.rint(size + v[2] * f32(ds)))


def sort_order(resp, size, octave, y, x, layer, row, col):
    """U8 + OURS-1 -> the permutation that sorts the list"""
    keys = [(-float(resp[k]), -float(size[k]), -int(octave[k]), -float(y[k]), float(x[k]), int(octave[k]), int(layer[k]),
             int(row[k]), int(col[k])) for k in range(len(resp))]
    return sorted(range(len(keys)), key=keys.__getitem__)


_GAUSS = {}


def gaussian_kernel(n, sigma):
    """U9: getGaussianKernel(n, sigma, CV_32F) for n > 7"""
    if (n, sigma) not in _GAUSS:
        scale2x = -0.5 / (sigma * sigma)
        c = np.zeros(n, f32)
        s = 0.0
        for i in range(n):
            x = i - (n - 1) * 0.5
            c[i] = f32(svo_exp(scale2x * x * x))
            s += float(c[i])
        s = 1.0 / s
        _GAUSS[(n, sigma)] = np.array([f32(float(v) * s) for v in c], f32)
    return _GAUSS[(n, sigma)]


def ori_samples():
    """U9 -> (ax, ay, weight) of the 113 samples"""
    G = gaussian_kernel(2 * ORI_RADIUS + 1, ORI_SIGMA)
    ax, ay, wt = [], [], []
    for i in range(-ORI_RADIUS, ORI_RADIUS + 1):
        for j in range(-ORI_RADIUS, ORI_RADIUS + 1):
            if i * i + j * j <= ORI_RADIUS * ORI_RADIUS:
                ax.append(i)
                ay.append(j)
                wt.append(G[i + ORI_RADIUS] * G[j + ORI_RADIUS])
    return np.array(ax, f32), np.array(ay, f32), np.array(wt, f32)


def desc_weights():
    G = gaussian_kernel(PATCH_SZ, DESC_SIGMA)
    return (G[:, None] * G[None, :]).astype(f32)


def scale_of(size):
    return f32(size) * f32(1.2) / f32(9.0)


def ori_positions(x, y, size, w, h):
    """U9 -> (fits, gws, s, xs, ys, valid) of one key point"""
    s = scale_of(size)
    ws = f32(PATCH_SZ + 1) * s
    if not (abs(f32(x)) <= 65536 and abs(f32(y)) <= 65536 and ws >= 21 and ws <= 65536):   # OURS-3
        return False, 0, s, None, None, None
    gws = 2 * int(np.rint(f32(2) * s))
    if h + 1 < gws or w + 1 < gws:
        return False, gws, s, None, None, None
    ax, ay, _ = ori_samples()
    off = f32(gws - 1) / f32(2)
    xs = np.rint(f32(x) + ax * s - off).astype(np.int64)
    ys = np.rint(f32(y) + ay * s - off).astype(np.int64)
    valid = (ys >= 0) & (ys < h + 1 - gws) & (xs >= 0) & (xs < w + 1 - gws)
    return True, gws, s, xs, ys, valid


def fits(x, y, size, w, h, upright=0):
    """U9: does the key point stay"""
    ok, _, _, _, _, valid = ori_positions(x, y, size, w, h)
    return bool(ok and (upright or valid.any()))


def orientation(S, x, y, size, w, h):
    """U9 -> angle (float32) or None when the key point is dropped; S: int64 integral image"""
    ok, gws, s, xs, ys, valid = ori_positions(x, y, size, w, h)
    if not ok or not valid.any():
        return None
    wt = ori_samples()[2][valid]
    xs, ys = xs[valid], ys[valid]
    X = calc_haar(S, ys, xs, resize_haar(GDX_S, 4, gws)) * wt
    Y = calc_haar(S, ys, xs, resize_haar(GDY_S, 4, gws)) * wt
    ang = np.rint(fast_atan2(Y, X)).astype(np.int64)
    d = np.abs(ang[None, :] - np.arange(0, 360, ORI_SEARCH_INC)[:, None])
    inside = (d < ORI_WIN // 2) | (d > 360 - ORI_WIN // 2)
    sumx, sumy = np.zeros(len(inside), f32), np.zeros(len(inside), f32)
    for j in range(len(X)):
        sumx = np.where(inside[:, j], sumx + X[j], sumx)
        sumy = np.where(inside[:, j], sumy + Y[j], sumy)
    mod = sumx * sumx + sumy * sumy
    k = int(np.argmax(mod))
    bestx, besty = (sumx[k], sumy[k]) if mod[k] > 0 else (f32(0), f32(0))
    return f32(fast_atan2(-besty, bestx))


def area_tab(win):
    """OURS-2 -> (fast k or 0, table rows (dst, src, alpha))"""
    scale = 1.0 / (21.0 / win)
    k = int(np.rint(scale))
    if abs(scale - k) < DBL_EPSILON:
        return k, [(d, d * k + t, f32(1)) for d in range(PATCH_SZ + 1) for t in range(k)]
    tab = []
    for dx in range(PATCH_SZ + 1):
        fsx1 = dx * scale
        fsx2 = fsx1 + scale
        cell = min(scale, win - fsx1)
        sx1, sx2 = int(np.ceil(fsx1)), int(np.floor(fsx2))
        sx2 = min(sx2, win - 1)
        sx1 = min(sx1, sx2)
        if sx1 - fsx1 > 1e-3:
            tab.append((dx, sx1 - 1, f32((sx1 - fsx1) / cell)))
        for sx in range(sx1, sx2):
            tab.append((dx, sx, f32(1.0 / cell)))
        if fsx2 - sx2 > 1e-3:
            tab.append((dx, sx2, f32(min(min(fsx2 - sx2, 1.0), cell) / cell)))
    return 0, tab


def window(grey, x, y, s, angle, upright):
    """U10 -> the win_size x win_size uint8 window"""
    h, w = grey.shape
    win = int(f32(PATCH_SZ + 1) * s)
    off = -f32(win - 1) / f32(2)
    if upright:
        sx, sy = int(np.rint(f32(x) + off)), int(np.rint(f32(y) - off))
        xs = np.clip(sx + np.arange(win), 0, w - 1)
        ys = np.clip(sy - np.arange(win), 0, h - 1)
        return grey[ys[None, :], xs[:, None]]
    rad = f32(angle) * f32(np.pi / 180)
    sin_dir, cos_dir = -f32(svo_sin(f64(rad))), f32(svo_cos(f64(rad)))
    start_x = f32(x) + off * cos_dir + off * sin_dir
    start_y = f32(y) - off * sin_dir + off * cos_dir
    row_x = np.add.accumulate(np.concatenate([[start_x], np.full(win - 1, sin_dir, f32)]).astype(f32))
    row_y = np.add.accumulate(np.concatenate([[start_y], np.full(win - 1, cos_dir, f32)]).astype(f32))
    px = np.empty((win, win), f64)
    py = np.empty((win, win), f64)
    px[:, 0], py[:, 0] = row_x, row_y
    px[:, 1:], py[:, 1:] = f64(cos_dir), -f64(sin_dir)
    px, py = np.add.accumulate(px, axis=1), np.add.accumulate(py, axis=1)
    ix, iy = np.floor(px).astype(np.int64), np.floor(py).astype(np.int64)
    inside = (ix >= 0) & (ix < w - 1) & (iy >= 0) & (iy < h - 1)
    cx, cy = np.clip(ix, 0, max(w - 2, 0)), np.clip(iy, 0, max(h - 2, 0))
    a, b = (px - ix).astype(f32), (py - iy).astype(f32)
    one = f32(1)
    g = grey.astype(f32)
    x1, y1 = np.minimum(cx + 1, w - 1), np.minimum(cy + 1, h - 1)
    v = g[cy, cx] * (one - a) * (one - b) + g[cy, x1] * a * (one - b) + g[y1, cx] * (one - a) * b + g[y1, x1] * a * b
    near = grey[np.clip(np.rint(py).astype(np.int64), 0, h - 1), np.clip(np.rint(px).astype(np.int64), 0, w - 1)]
    return np.where(inside, np.rint(v).astype(np.int64), near).astype(np.uint8)


def area_resize(win_img):
    """OURS-2 -> the 21 x 21 uint8 patch"""
    win = win_img.shape[0]
    k, tab = area_tab(win)
    n = PATCH_SZ + 1
    buf = np.zeros((win, n), f32)
    src = win_img.astype(f32)
    for d, s_, alpha in tab:
        buf[:, d] = buf[:, d] + src[:, s_] * alpha
    acc = np.zeros((n, n), f32)
    for d, s_, beta in tab:
        acc[d] = acc[d] + beta * buf[s_]
    if k == 2:
        return ((acc.astype(np.int64) + 2) >> 2).astype(np.uint8)
    if k:
        acc = acc.astype(np.int64).astype(f32) * (f32(1) / f32(k * k))
    return np.clip(np.rint(acc), 0, 255).astype(np.uint8)


def descriptor(grey, x, y, size, angle, upright=0):
    """U10 -> 64 float32"""
    patch = area_resize(window(grey, x, y, scale_of(size), angle, upright)).astype(np.int64)
    dw = desc_weights()
    p00, p01, p10, p11 = patch[:-1, :-1], patch[:-1, 1:], patch[1:, :-1], patch[1:, 1:]
    DX = (p01 - p00 + p11 - p10).astype(f32) * dw
    DY = (p10 - p00 + p11 - p01).astype(f32) * dw
    cx = DX.reshape(4, 5, 4, 5).transpose(0, 2, 1, 3).reshape(16, 25)
    cy = DY.reshape(4, 5, 4, 5).transpose(0, 2, 1, 3).reshape(16, 25)
    vec = np.zeros((16, 4), f32)
    for t in range(25):
        vec[:, 0] = vec[:, 0] + cx[:, t]
        vec[:, 1] = vec[:, 1] + cy[:, t]
        vec[:, 2] = vec[:, 2] + np.abs(cx[:, t])
        vec[:, 3] = vec[:, 3] + np.abs(cy[:, t])
    vec = vec.reshape(64)
    sq = 0.0
    for v in (vec * vec).astype(f64):
        sq += float(v)
    scale = f32(1.0 / (np.sqrt(sq) + float(FLT_EPSILON)))
    return vec * scale


def detect(img, hessian_threshold=100.0, n_octaves=4, n_octave_layers=3, extended=0, upright=0, planes=None):
    """U6 - U8 and the drops of U9 -> dict of arrays in output order (angle not yet set)"""
    assert not extended
    grey = to_grey(img)
    h, w = grey.shape
    dets, traces = planes if planes is not None else layers(grey, n_octaves, n_octave_layers)
    sizes, steps, lw, lh = layers_layout(w, h, n_octaves, n_octave_layers)
    thr = f32(hessian_threshold)
    nl = n_octave_layers + 2
    rec = []
    for o in range(n_octaves):
        for l in range(1, n_octave_layers + 1):
            L = o * nl + l
            size, step, pw, ph = sizes[L], steps[L], lw[L], lh[L]
            m = (sizes[L + 1] // 2) // step + 1
            if ph - 2 * m <= 0 or pw - 2 * m <= 0:
                continue
            c = dets[L][m:ph - m, m:pw - m]
            mask = c > thr
            for dl in (-1, 0, 1):
                for di in (-1, 0, 1):
                    for dj in (-1, 0, 1):
                        if dl or di or dj:
                            mask &= c > dets[L + dl][m + di:ph - m + di, m + dj:pw - m + dj]
            for i, j in zip(*np.nonzero(mask)):
                i, j = int(i) + m, int(j) + m
                N9 = [[dets[L + dl][i + di, j + dj] for di in (-1, 0, 1) for dj in (-1, 0, 1)] for dl in (-1, 0, 1)]
                half = f32(size - 1) * f32(0.5)
                cy_ = f32(step * (i - (size // 2) // step)) + half
                cx_ = f32(step * (j - (size // 2) // step)) + half
                ok, x, y, sz = interpolate(N9, step, size - sizes[L - 1], cx_, cy_, f32(size))
                if not ok or not fits(x, y, sz, w, h, upright):
                    continue
                t = traces[L][i, j]
                rec.append((x, y, sz, dets[L][i, j], o, int(t > 0) - int(t < 0), l, i, j))
    cols = list(zip(*rec)) if rec else [[] for _ in range(9)]
    x, y, sz, resp = (np.array(v, f32) for v in cols[:4])
    octv, lap, lay, row, col = (np.array(v, np.int32) for v in cols[4:])
    p = np.array(sort_order(resp, sz, octv, y, x, lay, row, col), np.int64)
    return dict(xy=np.stack([x[p], y[p]], axis=1).reshape(-1, 2), size=sz[p], response=resp[p], octave=octv[p],
                laplacian=lap[p], layer=lay[p], row=row[p], col=col[p])


def compute(img, xy, size, upright=0, descriptors=True):
    """detector->compute(img, keypoints) -> (angle [n], desc [n, 64], kept [n] uint8); a key point that is dropped (U9) has
    kept 0, angle -1 and a zero descriptor"""
    grey = to_grey(img)
    h, w = grey.shape
    S = integral(grey).astype(np.int64)
    xy = np.asarray(xy, f32).reshape(-1, 2)
    size = np.asarray(size, f32).reshape(-1)
    n = len(size)
    angle, desc, kept = np.full(n, -1, f32), np.zeros((n, 64), f32), np.zeros(n, np.uint8)
    for k in range(n):
        x, y, sz = xy[k, 0], xy[k, 1], size[k]
        if not fits(x, y, sz, w, h, upright):
            continue
        a = f32(270) if upright else orientation(S, x, y, sz, w, h)
        kept[k], angle[k] = 1, a
        if descriptors:
            desc[k] = descriptor(grey, x, y, sz, a, upright)
    return angle, desc, kept


def extract(img, descriptors=True, **params):
    """detectAndCompute -> the dict of detect plus angle and desc"""
    p = default_params(**params)
    kp = detect(img, **p)
    angle, desc, kept = compute(img, kp["xy"], kp["size"], p["upright"], descriptors)
    assert kept.all()
    kp["angle"], kp["desc"] = angle, desc
    return kp
