"""cv::goodFeaturesToTrack (OpenCV 3.2: cornerMinEigenVal / cornerHarris, the quality cut, the minimum-distance selection)
restated in numpy from the list below -- from memory of the 3.2 sources, not from csrc/gftt.hip and not from OpenCV, which is not
available here.  csrc/gftt.hip is held to this file bit for bit (tests/test_gpu_gftt.py); DESIGN.md section 10s and the README
state the same choices.  "recalled" = how 3.2 does it as far as memory goes, "choice" = fixed here because 3.2 leaves it open
or because the recollection is uncertain.

 G1  Input: 8-bit grey, or BGR converted with cvtColor's integer weights (1868 B + 9617 G + 4899 R + 8192) >> 14, the library's
     grey everywhere (recalled).  CV_32F input is not built.
 G2  cornerEigenValsVecs with aperture 3 (recalled): scale = 1 / (4 * blockSize * 255) formed in double (the product first, then
     the reciprocal); Dx and Dy = Sobel(CV_32F, ksize 3, scale, BORDER_REFLECT_101): the border is applied to the GREY image.
     The separable kernels are [-1 0 1] (difference) and [1 2 1] (smoothing); the scale is folded into the SMOOTHING kernel of
     both derivatives (getSobelKernels scales kx when dx == 0, else ky), whose float taps are k1 = (float)scale and
     k0 = (float)(2 * scale) = 2 * k1.  Order fixed here (choice; upstream's SIMD row / column filters are recalled only in
     shape): the ROW pass first, then the COLUMN pass, every operation in float, nothing fused:
         Dx: r = I(x + 1) - I(x - 1)                 (row pass, exact)
             dx = (r(y - 1) + r(y + 1)) * k1 + r(y) * k0     (column pass carries the scale)
         Dy: r = (I(x - 1) + I(x + 1)) * k1 + I(x) * k0      (row pass carries the scale)
             dy = r(y + 1) - r(y - 1)                (column pass)
 G3  Covariance: dx * dx, dx * dy, dy * dy in float (recalled).
 G4  boxFilter(CV_32F, blockSize x blockSize, centre anchor, normalize = false, BORDER_REFLECT_101) of the three product planes:
     the border is applied to the PRODUCT planes (a product outside the image is the product at the mirrored pixel, not the
     product of derivatives of a mirrored image).  Upstream accumulates float input in double with running column sums
     (recalled).  Choice: the double sum of the window's blockSize^2 floats in row-major order, rounded to float once.
     running_box() below is the running-column-sum order; tests/test_gftt_numpy.py records whether it changes a bit.
 G5  Corner measure, float, nothing fused (recalled): min-eigenvalue a = cxx * 0.5f, b = cxy, c = cyy * 0.5f,
     eig = (a + c) - sqrtf((a - c) * (a - c) + b * b); Harris ((cxx * cyy) - (cxy * cxy)) - ((float)k * (cxx + cyy)) * (cxx + cyy).
 G6  minMaxLoc: maxVal = the largest value of the plane, over the pixels whose mask byte is non-zero when a mask is given
     (recalled).  Choice: a mask that hides every pixel gives maxVal = 0.
 G7  threshold(TOZERO) with t = (float)(maxVal * qualityLevel), the product in double: eig = eig > t ? eig : 0 (recalled).
 G8  3 x 3 dilate of the thresholded plane; pixels outside the image never win (recalled).
 G9  A pixel is a candidate when 1 <= x <= w - 2, 1 <= y <= h - 2, eig != 0, eig == dilated and, with a mask, its mask byte is
     non-zero (recalled).  Every pixel of a plateau is a candidate.
 G10 Order: value descending; ties by row-major index DESCENDING (choice: the address comparator of later releases; 3.2's
     plain *a > *b under std::sort leaves ties unspecified).
 G11 minDistance >= 1 (recalled): cell = cvRound(minDistance) (round half to even), a grid of ceil(w / cell) x ceil(h / cell)
     cells; in order, a corner is rejected if an accepted corner in the 3 x 3 cells around its own has dx * dx + dy * dy <
     minDistance * minDistance, otherwise accepted; stop at maxCorners accepted when maxCorners > 0.  dx, dy and the left side
     are float; the right side is the double product minDistance * minDistance and the comparison promotes the left side, as
     the C++ expression does.  Choice: cell is cvRound(min(minDistance, 32768)) -- from a cell as large as the image on there
     is one cell and the result no longer depends on it -- so that any non-negative minDistance, infinity included, is legal.
 G12 minDistance < 1: the first maxCorners of the order, all of them if maxCorners <= 0 (recalled).
 G13 Output: (x, y) as floats in acceptance order; the response is the thresholded eig value (choice: goodFeaturesToTrack
     returns points only, GFTTDetector sets no response).

detect() also returns a record of the branches a fixture reaches (tests/gftt_fixtures.py proves each from it)."""
import numpy as np

F32 = np.float32
MAX_CELL = 32768.0


def to_gray(img):
    """G1"""
    img = np.asarray(img, np.uint8)
    if img.ndim == 2:
        return img.copy()
    if img.shape[2] == 1:
        return img[..., 0].copy()
    b, g, r = (img[..., k].astype(np.int64) for k in range(3))
    return ((1868 * b + 9617 * g + 4899 * r + 8192) >> 14).astype(np.uint8)


def cv_round(v):
    """cvRound: to nearest, halves to even"""
    return int(np.rint(np.float64(v)))


def reflect101(p, n):
    """cv::borderInterpolate(p, n, BORDER_REFLECT_101)"""
    if n == 1:
        return 0
    while p < 0 or p >= n:
        p = -p if p < 0 else 2 * n - 2 - p
    return p


def _padded(plane, r):
    """plane with r mirrored rows / columns on every side"""
    h, w = plane.shape
    iy = [reflect101(y, h) for y in range(-r, h + r)]
    ix = [reflect101(x, w) for x in range(-r, w + r)]
    return plane[np.ix_(iy, ix)]


def sobel_scale(block_size):
    """G2: (k1, k0), the two distinct taps of the scaled smoothing kernel"""
    scale = 1.0 / (4.0 * block_size * 255.0)
    return F32(scale), F32(2.0 * scale)


def derivatives(gray, block_size):
    """G2 -> (dx, dy) float32"""
    k1, k0 = sobel_scale(block_size)
    f = _padded(gray, 1).astype(F32)
    r = f[:, 2:] - f[:, :-2]
    dx = (r[:-2] + r[2:]) * k1 + r[1:-1] * k0
    r = (f[:, :-2] + f[:, 2:]) * k1 + f[:, 1:-1] * k0
    dy = r[2:] - r[:-2]
    assert dx.dtype == F32 and dy.dtype == F32
    return dx, dy


def box(plane, block_size):
    """G4: the double sum of the window in row-major order, rounded to float once"""
    h, w = plane.shape
    p = _padded(plane, block_size // 2).astype(np.float64)
    acc = np.zeros((h, w), np.float64)
    for j in range(block_size):
        for i in range(block_size):
            acc = acc + p[j:j + h, i:i + w]
    return acc.astype(F32)


def running_box(plane, block_size):
    """The order upstream's ColumnSum gives (recalled): per column the running double sum over the window's rows (add the row that
    enters, subtract the row that leaves, starting from the first window's rows summed top down), over row sums that are the
    double sum of blockSize floats left to right."""
    h, w = plane.shape
    p = _padded(plane, block_size // 2).astype(np.float64)
    rows = np.zeros((p.shape[0], w), np.float64)
    for i in range(block_size):
        rows = rows + p[:, i:i + w]
    out = np.zeros((h, w), np.float64)
    s = np.zeros(w, np.float64)
    for j in range(block_size - 1):
        s = s + rows[j]
    for y in range(h):
        s = s + rows[y + block_size - 1]
        out[y] = s
        s = s - rows[y]
    return out.astype(F32)


def response(img, block_size=3, use_harris=False, k=0.04, box_fn=box):
    """G1 ... G5: the plane before thresholding (svo_gftt_response)"""
    g = to_gray(img)
    dx, dy = derivatives(g, block_size)
    cxx, cxy, cyy = box_fn(dx * dx, block_size), box_fn(dx * dy, block_size), box_fn(dy * dy, block_size)
    if use_harris:
        kf = F32(k)
        return ((cxx * cyy) - (cxy * cxy)) - (kf * (cxx + cyy)) * (cxx + cyy)
    a, b, c = cxx * F32(0.5), cxy, cyy * F32(0.5)
    return (a + c) - np.sqrt((a - c) * (a - c) + b * b)


def candidates(eig, quality_level, mask=None):
    """G6 ... G10 -> (index [n] row-major, value [n]) in the total order, and the record"""
    h, w = eig.shape
    shown = np.ones((h, w), bool) if mask is None else np.asarray(mask) != 0
    max_val = float(eig[shown].max()) if shown.any() else 0.0
    t = F32(max_val * float(quality_level))
    thr = np.where(eig > t, eig, F32(0)).astype(F32)
    pad = np.full((h + 2, w + 2), -np.inf, F32)
    pad[1:-1, 1:-1] = thr
    dil = np.max([pad[j:j + h, i:i + w] for j in range(3) for i in range(3)], axis=0)
    ok = (thr != 0) & (thr == dil) & shown
    ok[[0, -1], :] = False
    ok[:, [0, -1]] = False
    idx = np.flatnonzero(ok)
    val = thr.ravel()[idx]
    order = np.lexsort((-idx, -val.astype(np.float64)))
    idx, val = idx[order], val[order]
    y, x = np.divmod(idx, w)
    touching = False
    if len(idx):
        plane = np.zeros((h + 2, w + 2), bool)
        plane[y + 1, x + 1] = True
        touching = bool(max((plane[1:-1, 1:-1] & plane[1 + j:h + 1 + j, 1 + i:w + 1 + i]).any()
                            for j, i in ((0, 1), (1, 0), (1, 1), (1, -1))))
    rec = dict(max_val=max_val, threshold=float(t), n_candidates=len(idx), plateau=touching,
               ties=int(len(val) - len(np.unique(val))), x_min=int(x.min()) if len(x) else None,
               x_max=int(x.max()) if len(x) else None)
    return idx, val, rec


def select(xs, ys, min_distance, max_corners, w, h):
    """G11 / G12 on candidates in order -> the positions (in the order) of the accepted ones"""
    n = len(xs)
    if min_distance < 1:
        return list(range(n if max_corners <= 0 else min(n, max_corners)))
    cell = cv_round(min(float(min_distance), MAX_CELL))
    gw, gh = (w + cell - 1) // cell, (h + cell - 1) // cell
    md2 = float(min_distance) * float(min_distance)
    grid = {}
    out = []
    for i in range(n):
        x, y = int(xs[i]), int(ys[i])
        cx, cy = x // cell, y // cell
        good = True
        for yy in range(max(cy - 1, 0), min(cy + 1, gh - 1) + 1):
            for xx in range(max(cx - 1, 0), min(cx + 1, gw - 1) + 1):
                for (px, py) in grid.get((xx, yy), ()):
                    dx, dy = F32(x) - F32(px), F32(y) - F32(py)
                    if float(dx * dx + dy * dy) < md2:
                        good = False
        if good:
            grid.setdefault((cx, cy), []).append((x, y))
            out.append(i)
            if max_corners > 0 and len(out) == max_corners:
                break
    return out


def select_all_pairs(xs, ys, min_distance, max_corners):
    """The greedy selection without a grid, O(n^2): what G11 must equal"""
    n = len(xs)
    if min_distance < 1:
        return list(range(n if max_corners <= 0 else min(n, max_corners)))
    md2 = float(min_distance) * float(min_distance)
    out = []
    for i in range(n):
        dx, dy = F32(xs[i]) - np.asarray(xs, F32)[out], F32(ys[i]) - np.asarray(ys, F32)[out]
        if not ((dx * dx + dy * dy).astype(np.float64) < md2).any():
            out.append(i)
            if max_corners > 0 and len(out) == max_corners:
                break
    return out


def selection_rounds(xs, ys, min_distance):
    """Rounds of the lock-step form of G11 (every undecided corner is rejected if an accepted one lies within the distance,
    accepted if no undecided corner of earlier rank does, waits otherwise) -> (accepted positions, rounds)"""
    n = len(xs)
    if min_distance < 1 or n == 0:
        return list(range(n)), 0
    x, y = np.asarray(xs, F32), np.asarray(ys, F32)
    dx, dy = x[:, None] - x[None, :], y[:, None] - y[None, :]
    near = (dx * dx + dy * dy).astype(np.float64) < float(min_distance) * float(min_distance)
    np.fill_diagonal(near, False)
    earlier = np.tri(n, n, -1, dtype=bool)                    # [i, j]: j ranks before i
    state = np.zeros(n, int)                                  # 0 undecided, 1 accepted, 2 rejected
    rounds = 0
    while (state == 0).any():
        rej = (near & (state == 1)[None, :]).any(axis=1)
        wait = (near & earlier & (state == 0)[None, :]).any(axis=1)
        new = np.where(rej, 2, np.where(wait, 0, 1))
        state = np.where(state == 0, new, state)
        rounds += 1
    return list(np.flatnonzero(state == 1)), rounds


def detect(img, max_corners=1000, quality_level=0.01, min_distance=1.0, mask=None, block_size=3, use_harris=False, k=0.04):
    """goodFeaturesToTrack -> (xy [n, 2] float32, response [n] float32, record)"""
    g = to_gray(img)
    h, w = g.shape
    empty = (np.zeros((0, 2), F32), np.zeros(0, F32))
    if w < 3 or h < 3:
        return (*empty, dict(n_candidates=0, too_small=True, max_val=0.0, n_accepted=0))
    eig = response(g, block_size, use_harris, k)
    idx, val, rec = candidates(eig, quality_level, mask)
    ys, xs = np.divmod(idx, w)
    keep = select(xs, ys, min_distance, max_corners, w, h)
    free = select(xs, ys, min_distance, 0, w, h)
    rec.update(too_small=False, n_accepted=len(keep), n_accepted_unbounded=len(free), negative=int((eig < 0).sum()),
               rounds=selection_rounds(xs, ys, min_distance)[1] if len(xs) <= 2000 else None,   # all pairs: small sets only
               cell=cv_round(min(float(min_distance), MAX_CELL)) if min_distance >= 1 else 0)
    xy = np.stack([xs[keep], ys[keep]], axis=1).astype(F32).reshape(-1, 2)
    return xy, val[keep].astype(F32), rec
