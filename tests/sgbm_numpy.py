"""A numpy restatement of OpenCV's dense stereo matcher as the reference calls it (src/StereoCV.cpp:21-59, 227-250):
``StereoSGBM`` in ``MODE_SGBM`` (``computeDisparitySGBM`` + ``StereoSGBMImpl::compute``), ``filterSpeckles``,
``stereoRectify``'s ``Q`` and ``reprojectImageTo3D``.  It is the checker of csrc/sgbm.hip, in the role lk_numpy.py has
for the tracker: every test compares the device result with it bit for bit.

OpenCV version assumed: 3.2 (the era SURVEY.md dates the reference to).  Neither OpenCV nor its sources are available to
this project, so what follows is restated from recollection of modules/calib3d/src/stereosgbm.cpp and calibration.cpp,
not copied.  The points that are recollections rather than citations (DESIGN.md section 10 keeps the same list):

 R1  pre-filter cap: ``ftzero = max(preFilterCap, 15) | 1`` (61 for the reference's 60), clip table
     ``tab[v] = (uchar)(clamp(v, -ftzero, ftzero) + ftzero)``.  The table is recalled as an array of PixType
     (uchar), so for a cap above 127 (ftzero >= 129) the entries wrap modulo 256, and so does the border value
     ``tab[0] = (uchar)ftzero`` of R2 in both channels.  That range rests on this recollection alone; no OpenCV was
     run for it.
 R2  pre-filter: ``v = 2 (I[y][x+1] - I[y][x-1]) + I[y-1][x+1] - I[y-1][x-1] + I[y+1][x+1] - I[y+1][x-1]`` for
     x in [1, w-1); rows y-1 / y+1 replaced by row y itself at the top / bottom edge; columns 0 and w-1 of the derivative
     row are ``tab[0] = ftzero``.  The second cost channel is the raw intensity, whose columns 0 and w-1 are ALSO set to
     ``ftzero`` (the border loop of calcPixelCostBT runs over both channels).
 R3  Birchfield-Tomasi: per channel, half-sample min / max ``v0 / v1`` of the right row (neighbour averages with C integer
     division, a missing neighbour replaced by the pixel itself), the same ``u0 / u1`` of the left row;
     ``c0 = max(0, u - v1, v0 - u)``, ``c1 = max(0, v - u1, u0 - v)``, cost ``+= min(c0, c1) >> diff_scale`` with
     diff_scale 0 for the derivative channel and 2 for the intensity channel.  Only band columns
     ``[minX1, maxX1)``, ``minX1 = max(maxD, 0)``, ``maxX1 = w + min(minD, 0)``, are costed.
 R4  block sum, horizontal: ``hsum[x] = sum_{j=-SW2..SW2} pix[clamp(x + j, 0, width1 - 1)]`` over BAND columns (the
     running sum replicates the band's edge columns).  3.2 reads past the band for its first column when SW2 >= width1;
     the clamp is taken there.
 R5  block sum, vertical, as 3.2's single-row C buffer does it: ``C[0] = (SH2 + 1) hsum[0] + sum_{k=1..SH2} hsum[min(k,
     h - 1)]``; for y > 0 ``C[y] = C[y-1] + hsum[y + SH2] - hsum[max(y - SH2 - 1, 0)]`` only while y + SH2 < h -- the
     last SH2 rows keep the C of the row before (the update sits inside 3.2's ``if (k < height)``).  The band's FIRST
     column is never updated after row 0 (3.2's update loop starts at x = D; later releases add the missing column).
     C is stored as int16 and starts at P2 (the buffer is pre-filled with P2, which the recurrence subtracts again).
 R6  path recurrence ``Lr = C + min(Lr'[d], Lr'[d-1] + P1, Lr'[d+1] + P1, minLr' + P2) - (minLr' + P2)``, with
     ``Lr'[-1] = Lr'[D] = SHRT_MAX``; Lr and minLr are stored as int16; a path starts at the band's edge / the first
     row with ``Lr' = 0, minLr' = 0``.  Directions of MODE_SGBM: left->right, (x-1, y-1), (x, y-1), (x+1, y-1) in the
     top-to-bottom sweep, right->left inside the winner-take-all loop.
 R7  ``S = sat16(L0 + L1 + L2 + L3)`` in the sweep, then ``S = sat16(S + L4)`` in the WTA loop; the best disparity is
     the FIRST d with the smallest S (strict <, start SHRT_MAX: an all-saturated pixel gets d = -1).
 R8  uniqueness: the pixel is dropped when some d has ``S[d] (100 - ratio) < minS 100`` and ``|d - best| > 1``
     (a negative ratio reads as 10).  A dropped pixel updates nothing.
 R9  disp2: ``x2 = x - (best + minD)``; updated when ``disp2cost[x2] > minS`` while x runs from the band's right edge
     to its left -- of equal-cost left pixels the RIGHTMOST wins.  disp2 starts at ``(minD - 1) * 16`` (the scaled
     invalid value, compared below against the unscaled minD) and disp2cost at SHRT_MAX.
 R10 sub-pixel: for 0 < d < D-1, ``denom2 = max(S[d-1] + S[d+1] - 2 S[d], 1)``,
     ``d16 = 16 d + ((S[d-1] - S[d+1]) 16 + denom2) / (2 denom2)`` with C division (truncation toward zero); else 16 d.
     Stored ``d16 + 16 minD``.
 R11 left-right check: ``_d = d16 >> 4``, ``d_ = (d16 + 15) >> 4``; the pixel is invalidated only when BOTH
     ``x - _d`` and ``x - d_`` are inside the image, both disp2 entries are ``>= minD`` and both differ from ``_d`` /
     ``d_`` by more than disp12MaxDiff; ``disp12MaxDiff <= 0`` reads as 1 (``params.disp12MaxDiff > 0 ? .. : 1``).
 R12 ``StereoSGBMImpl::compute`` applies ``medianBlur(disp, disp, 3)`` (replicated border) after the matcher and
     before the speckle filter -- recalled from 2.4's ``StereoSGBM::operator()`` and kept in 3.x's ``compute``.
 R13 filterSpeckles: 4-connected components of pixels != newVal, neighbours joined when ``|a - b| <= maxDiff``;
     components with ``count <= maxSpeckleSize`` become newVal.  newVal ``(minD - 1) 16``, maxDiff ``16 speckleRange``.
 R14 P1 <= 0 reads as 2, P2 <= 0 as 5, then ``P2 = max(P2, P1 + 1)`` (the C ABI refuses p2 <= p1 anyway).
 R15 stereoRectify for equal K, zero distortion, R = I, T = (tx, 0, 0), CALIB_ZERO_DISPARITY, alpha -1, same size:
     R1 = R2 = I, ``fc_new = fy``; the principal point is ``(n - 1) / 2 - mean(projected corners)`` where the four
     image corners go through undistortPoints ((u - cx) * (1 / fx), stored float) and projectPoints (fc_new * x, stored
     float), averaged in double; ``(n - 1) / 2`` in double.  ``Q = [[1, 0, 0, -ccx], [0, 1, 0, -ccy], [0, 0, 0, fc_new],
     [0, 0, -1 / tx, (ccx0 - ccx1) / tx]]``.
 R16 reprojectImageTo3D (handleMissingValues false): ``X = (qx + Q02 d) iW`` ... with ``iW = 1 / (qw + Q32 d)`` in
     double, stored float.  OpenCV accumulates ``qx += Q00`` along x; both the kernel and this restatement use the
     closed form ``qx = (Q01 y + Q03) + Q00 x``.  For KITTI's 1241 columns the two differ by at most 1241 half-ulps of
     a value below 2048 (< 3e-10 absolute), i.e. only where a float rounding lands within that of a tie.

The reference's own call: ``t = +baseline`` gives ``Q32 = -1 / baseline`` and ``Z = fc_new / (-d / baseline) < 0`` for
every positive disparity; disparity 0 (the invalid value of minDisparity 1) gives W = +0, Z = +inf.  Its window
``Z > 5 or Z <= 0.01`` therefore keeps nothing from a valid pixel; NaN would be kept (both comparisons false) but Z is
``fc_new * iW`` and never NaN with these Q.  The conventional ``tx = -baseline`` gives positive Z.
"""
from __future__ import annotations

import dataclasses

import numpy as np

SHRT_MAX = 32767
DISP_SHIFT, DISP_SCALE = 4, 16


@dataclasses.dataclass
class Params:
    """StereoSGBM::create's arguments, defaults = the reference's call (src/StereoCV.cpp:40-51)."""
    min_disparity: int = 1
    num_disparities: int = 96
    block_size: int = 7
    p1: int = 24
    p2: int = 96
    disp12_max_diff: int = 0
    pre_filter_cap: int = 60
    uniqueness_ratio: int = 0
    speckle_window_size: int = 3000
    speckle_range: int = 5
    mode: int = 0


def cv_gray(img: np.ndarray) -> np.ndarray:
    """cvtColor(BGR2GRAY) with OpenCV's fixed-point weights (the library's cv_gray_kernel recipe)."""
    if img.ndim == 2:
        return img
    if img.shape[2] == 1:
        return img[..., 0]
    b, g, r = (img[..., k].astype(np.int64) for k in range(3))
    return ((1868 * b + 9617 * g + 4899 * r + 8192) >> 14).astype(np.uint8)


def c_div(a, b):
    """C integer division (truncation toward zero) of int arrays; b > 0."""
    a = np.asarray(a, np.int64)
    q = np.abs(a) // b
    return np.where(a < 0, -q, q)


def _prefilter_rows(img: np.ndarray, ftzero: int):
    """(derivative channel, intensity channel) int32 h x w holding uint8 values (R1, R2): the table entries and the
    border value tab[0] are stored as uchar, so they wrap modulo 256 once ftzero exceeds 127."""
    I = img.astype(np.int32)
    h, w = I.shape
    up = np.concatenate([I[:1], I[:-1]], 0)
    dn = np.concatenate([I[1:], I[-1:]], 0)
    der = np.full((h, w), ftzero & 255, np.int32)
    inten = np.full((h, w), ftzero & 255, np.int32)
    if w > 2:
        v = (I[:, 2:] - I[:, :-2]) * 2 + up[:, 2:] - up[:, :-2] + dn[:, 2:] - dn[:, :-2]
        der[:, 1:-1] = (np.clip(v, -ftzero, ftzero) + ftzero) & 255
        inten[:, 1:-1] = I[:, 1:-1]
    return der, inten


def _half_minmax(row: np.ndarray):
    """(v0, v1): min / max of the pixel and its half-way averages with existing neighbours (R3), last axis = x."""
    w = row.shape[-1]
    left = np.concatenate([row[..., :1], row[..., :-1]], -1)
    right = np.concatenate([row[..., 1:], row[..., -1:]], -1)
    vl = (row + left) // 2
    vr = (row + right) // 2
    if w > 0:
        vl[..., 0] = row[..., 0]
        vr[..., -1] = row[..., -1]
    return np.minimum(np.minimum(vl, vr), row), np.maximum(np.maximum(vl, vr), row)


def pixel_cost(left: np.ndarray, right: np.ndarray, p: Params):
    """calcPixelCostBT for every row: int32 h x width1 x D (band columns only)."""
    minD, D = p.min_disparity, p.num_disparities
    maxD = minD + D
    h, w = left.shape
    minX1, maxX1 = max(maxD, 0), w + min(minD, 0)
    width1 = maxX1 - minX1
    ftzero = max(p.pre_filter_cap, 15) | 1
    out = np.zeros((h, max(width1, 0), D), np.int32)
    if width1 <= 0:
        return out
    xs = np.arange(minX1, maxX1)
    xr = xs[:, None] - (minD + np.arange(D))[None, :]   # right-image column of (x, d), always inside [0, w)
    for chan, shift in zip(range(2), (0, 2)):
        L = _prefilter_rows(left, ftzero)[chan]
        R = _prefilter_rows(right, ftzero)[chan]
        u0, u1 = _half_minmax(L)
        v0, v1 = _half_minmax(R)
        u, uu0, uu1 = L[:, xs][:, :, None], u0[:, xs][:, :, None], u1[:, xs][:, :, None]
        v, vv0, vv1 = R[:, xr], v0[:, xr], v1[:, xr]
        c0 = np.maximum(np.maximum(0, u - vv1), vv0 - u)
        c1 = np.maximum(np.maximum(0, v - uu1), uu0 - v)
        out += np.minimum(c0, c1) >> shift
    return out


def block_cost(pix: np.ndarray, p: Params) -> np.ndarray:
    """C of R4 / R5 (int16, includes the +P2 offset): h x width1 x D."""
    h, width1, D = pix.shape
    SW2 = SH2 = p.block_size // 2
    P2 = _penalties(p)[1]
    idx = np.clip(np.arange(width1)[:, None] + np.arange(-SW2, SW2 + 1)[None, :], 0, width1 - 1)
    hsum = pix[:, idx, :].sum(2)                          # h x width1 x D, int
    C = np.empty((h, width1, D), np.int16)
    c = np.full((width1, D), P2, np.int64)
    for k in range(SH2 + 1):
        c += hsum[min(k, h - 1)] * (SH2 + 1 if k == 0 else 1)
    C[0] = c.astype(np.int16)
    for y in range(1, h):
        prev = C[y - 1].astype(np.int64)
        if y + SH2 < h:
            cur = prev + hsum[y + SH2] - hsum[max(y - SH2 - 1, 0)]
            cur[0] = prev[0]
            C[y] = cur.astype(np.int16)
        else:
            C[y] = C[y - 1]
    return C


def _penalties(p: Params):
    P1 = p.p1 if p.p1 > 0 else 2
    P2 = max(p.p2 if p.p2 > 0 else 5, P1 + 1)
    return P1, P2


def path_step(Cx: np.ndarray, Lp: np.ndarray, minLp: np.ndarray, P1: int, P2: int):
    """One step of R6 for a stack of lines.  Cx, Lp: (n, D) int16; minLp: (n,) int16.
    Returns (L as int, stored int16 L, stored int16 minL)."""
    n, D = Lp.shape
    Lp = Lp.astype(np.int64)
    pad = np.full((n, D + 2), SHRT_MAX, np.int64)
    pad[:, 1:-1] = Lp
    delta = minLp.astype(np.int64)[:, None] + P2
    m = np.minimum(np.minimum(Lp, pad[:, :-2] + P1), np.minimum(pad[:, 2:] + P1, delta))
    L = Cx.astype(np.int64) + m - delta
    return L, L.astype(np.int16), L.min(1).astype(np.int16)


def path_costs(C: np.ndarray, p: Params, direction: int) -> np.ndarray:
    """The int L of one direction at every (y, x, d).  direction: 0 left->right, 1 from (x-1, y-1), 2 from (x, y-1),
    3 from (x+1, y-1), 4 right->left."""
    h, width1, D = C.shape
    P1, P2 = _penalties(p)
    out = np.empty((h, width1, D), np.int64)
    if direction in (0, 4):
        Lp = np.zeros((h, D), np.int16)
        mp = np.zeros(h, np.int16)
        xs = range(width1) if direction == 0 else range(width1 - 1, -1, -1)
        for x in xs:
            L, Lp, mp = path_step(C[:, x], Lp, mp, P1, P2)
            out[:, x] = L
        return out
    dx = {1: 1, 2: 0, 3: -1}[direction]
    Lp = np.zeros((width1, D), np.int16)
    mp = np.zeros(width1, np.int16)
    for y in range(h):
        # predecessor of x is x - dx in the previous row; outside the band: Lr' = 0, minLr' = 0
        Ls = np.zeros((width1, D), np.int16)
        ms = np.zeros(width1, np.int16)
        if dx == 0:
            Ls, ms = Lp, mp
        elif dx == 1:
            Ls[1:], ms[1:] = Lp[:-1], mp[:-1]
        else:
            Ls[:-1], ms[:-1] = Lp[1:], mp[1:]
        L, Lp, mp = path_step(C[y], Ls, ms, P1, P2)
        out[y] = L
    return out


def aggregate(C: np.ndarray, p: Params) -> np.ndarray:
    """S of R7 (int64 holding int16 values)."""
    S = np.zeros(C.shape, np.int64)
    for r in range(4):
        S += path_costs(C, p, r)
    S = np.clip(S, -32768, SHRT_MAX)
    return np.clip(S + path_costs(C, p, 4), -32768, SHRT_MAX)


def wta(S: np.ndarray, p: Params, w: int) -> np.ndarray:
    """R7-R11: h x w int16 disparities x16 (before the median and the speckle filter)."""
    h, width1, D = S.shape
    minD = p.min_disparity
    maxD = minD + D
    minX1 = max(maxD, 0)
    invalid = (minD - 1) * DISP_SCALE
    ratio = p.uniqueness_ratio if p.uniqueness_ratio >= 0 else 10
    maxdiff = p.disp12_max_diff if p.disp12_max_diff > 0 else 1
    disp = np.full((h, w), invalid, np.int64)
    if width1 <= 0:
        return disp.astype(np.int16)
    minS = S.min(2)
    best = S.argmin(2)
    best = np.where(minS >= SHRT_MAX, -1, best)
    minS = np.where(minS >= SHRT_MAX, SHRT_MAX, minS)
    dd = np.arange(D)[None, None, :]
    bad = ((S * (100 - ratio) < minS[..., None] * 100) & (np.abs(best[..., None] - dd) > 1)).any(2)
    ok = ~bad
    # sub-pixel (R10)
    bc = np.clip(best, 1, max(D - 2, 1))
    Sm = np.take_along_axis(S, np.clip(bc - 1, 0, D - 1)[..., None], 2)[..., 0]
    S0 = np.take_along_axis(S, np.clip(bc, 0, D - 1)[..., None], 2)[..., 0]
    Sp = np.take_along_axis(S, np.clip(bc + 1, 0, D - 1)[..., None], 2)[..., 0]
    denom2 = np.maximum(Sm + Sp - 2 * S0, 1)
    inner = (best > 0) & (best < D - 1)
    d16 = np.where(inner, best * DISP_SCALE + c_div((Sm - Sp) * DISP_SCALE + denom2, 2 * denom2), best * DISP_SCALE)
    band = np.where(ok, d16 + minD * DISP_SCALE, invalid)
    disp[:, minX1:minX1 + width1] = band
    # disp2 (R9): per right column the minimum cost, the rightmost left pixel on ties
    xs = np.arange(width1)
    for y in range(h):
        disp2 = np.full(w, invalid, np.int64)
        cost2 = np.full(w, SHRT_MAX, np.int64)
        sel = ok[y] & (best[y] >= 0)
        x2 = xs + minX1 - best[y] - minD
        for x in np.nonzero(sel)[0][::-1]:
            if cost2[x2[x]] > minS[y, x]:
                cost2[x2[x]] = minS[y, x]
                disp2[x2[x]] = best[y, x] + minD
        row = disp[y]
        for x in range(minX1, minX1 + width1):
            d1 = row[x]
            if d1 == invalid:
                continue
            _d, d_ = d1 >> DISP_SHIFT, (d1 + DISP_SCALE - 1) >> DISP_SHIFT
            _x, x_ = x - _d, x - d_
            if (0 <= _x < w and disp2[_x] >= minD and abs(disp2[_x] - _d) > maxdiff and
                    0 <= x_ < w and disp2[x_] >= minD and abs(disp2[x_] - d_) > maxdiff):
                row[x] = invalid
    return disp.astype(np.int16)


def median3(disp: np.ndarray) -> np.ndarray:
    """medianBlur(ksize 3) with a replicated border (R12)."""
    h, w = disp.shape
    pad = np.pad(disp.astype(np.int32), 1, mode="edge")
    win = np.stack([pad[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)], 0)
    return np.sort(win, 0)[4].astype(np.int16)


def filter_speckles(disp: np.ndarray, new_val: int, max_size: int, max_diff: int) -> np.ndarray:
    """filterSpeckles (R13) as a connected-components problem."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components

    d = disp.astype(np.int64)
    h, w = d.shape
    valid = d != new_val
    ids = np.arange(h * w).reshape(h, w)
    rows, cols = [], []
    for a, b, da, db, va, vb in ((ids[:, :-1], ids[:, 1:], d[:, :-1], d[:, 1:], valid[:, :-1], valid[:, 1:]),
                                 (ids[:-1], ids[1:], d[:-1], d[1:], valid[:-1], valid[1:])):
        m = va & vb & (np.abs(da - db) <= max_diff)
        rows.append(a[m])
        cols.append(b[m])
    r, c = np.concatenate(rows), np.concatenate(cols)
    g = coo_matrix((np.ones(r.size, np.int8), (r, c)), shape=(h * w, h * w))
    _, lab = connected_components(g, directed=False)
    size = np.bincount(lab, minlength=lab.max() + 1)
    small = (size[lab] <= max_size).reshape(h, w) & valid
    out = disp.copy()
    out[small] = new_val
    return out


def sgbm(left: np.ndarray, right: np.ndarray, p: Params | None = None, stages: dict | None = None) -> np.ndarray:
    """StereoSGBM::compute(left, right) -> int16 h x w (disparity x 16).  BGR or grey uint8 inputs."""
    p = p or Params()
    gl, gr = cv_gray(np.asarray(left)), cv_gray(np.asarray(right))
    h, w = gl.shape
    pix = pixel_cost(gl, gr, p)
    if pix.shape[1] > 0:
        C = block_cost(pix, p)
        S = aggregate(C, p)
    else:
        C = S = np.zeros((h, 0, p.num_disparities), np.int64)
    raw = wta(S, p, w)
    disp = median3(raw)
    if stages is not None:
        stages.update(pix=pix, C=C, S=S, raw=raw, median=disp.copy())
    if p.speckle_window_size > 0:
        disp = filter_speckles(disp, (p.min_disparity - 1) * DISP_SCALE, p.speckle_window_size,
                               DISP_SCALE * p.speckle_range)
    return disp


def stereo_rectify_q(fx, fy, cx, cy, tx, w, h) -> np.ndarray:
    """Q of stereoRectify (R15), 4 x 4 float64."""
    f32 = np.float32
    fc_new = fy
    ifx, ify = 1.0 / fx, 1.0 / fy
    corners = [(0.0, 0.0), (float(w - 1), 0.0), (0.0, float(h - 1)), (float(w - 1), float(h - 1))]
    sx = sy = 0.0
    for u, v in corners:
        xu = float(f32((float(f32(u)) - cx) * ifx))
        yu = float(f32((float(f32(v)) - cy) * ify))
        sx += float(f32(xu * fc_new + 0.0))
        sy += float(f32(yu * fc_new + 0.0))
    ccx = (w - 1) / 2.0 - sx * 0.25
    ccy = (h - 1) / 2.0 - sy * 0.25
    Q = np.zeros((4, 4))
    Q[0, 0] = Q[1, 1] = 1.0
    Q[0, 3], Q[1, 3], Q[2, 3] = -ccx, -ccy, fc_new
    Q[3, 2] = -1.0 / tx
    Q[3, 3] = (ccx - ccx) / tx
    return Q


def reproject(disp: np.ndarray, image: np.ndarray, Q: np.ndarray, disp_scale: float = 1.0, z_min: float = 0.01,
              z_max: float = 5.0, flip_y: bool = True):
    """convertTo(CV_32F, disp_scale) + reprojectImageTo3D + the window / flip / colour loop of reprojectDisparity
    (src/StereoCV.cpp:227-250): -> (xyz float32 n x 3, bgr float32 n x 3) in row-major order."""
    h, w = disp.shape
    q = np.asarray(Q, np.float64).reshape(4, 4)
    d = (disp.astype(np.float32) * np.float32(disp_scale)).astype(np.float64)
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        qx = (q[0, 1] * yy + q[0, 3]) + q[0, 0] * xx
        qy = (q[1, 1] * yy + q[1, 3]) + q[1, 0] * xx
        qz = (q[2, 1] * yy + q[2, 3]) + q[2, 0] * xx
        qw = (q[3, 1] * yy + q[3, 3]) + q[3, 0] * xx
        iW = 1.0 / (qw + q[3, 2] * d)
        X = ((qx + q[0, 2] * d) * iW).astype(np.float32)
        Y = ((qy + q[1, 2] * d) * iW).astype(np.float32)
        Z = ((qz + q[2, 2] * d) * iW).astype(np.float32)
        skip = (Z > np.float32(z_max)) | (Z <= np.float32(z_min))
    keep = ~skip
    if flip_y:
        Y = -Y
    xyz = np.stack([X[keep], Y[keep], Z[keep]], 1).astype(np.float32)
    img = image if image.ndim == 3 else image[..., None]
    if img.shape[2] == 1:
        img = np.repeat(img, 3, 2)
    bgr = img[keep].astype(np.float32)
    return xyz, bgr
