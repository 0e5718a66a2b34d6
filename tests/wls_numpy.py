"""The disparity WLS filter the reference's author wrote around the matcher (src/StereoCV.cpp:25-28,51-59, commented out
upstream): ximgproc::createDisparityWLSFilter(matcher) + createRightMatcher(matcher) + filter(disp, grey, out, rdisp),
restated operation by operation.  OpenCV / ximgproc are absent here; every point below is either RECALLED from ximgproc 3.2
(disparity_filters.cpp / fgs_filter.cpp) or OURS (decided here, the library on the same side).  DESIGN.md section 10h
carries the same list.

W1  RECALLED  createRightMatcher (SGBM case): min_disparity = -(minD + numD) + 1, the same num_disparities, block_size,
    p1, p2, pre_filter_cap and mode, uniqueness_ratio 0, disp12_max_diff 1000000, speckle window / range 0; run as
    compute(right, left); its disparities are <= 0 (x 16), its invalid value (min_disparity - 1) * 16 of its own.
W2  RECALLED  createDisparityWLSFilter(matcher): lambda 8000, sigma_color 1.5, use_confidence, LRC_thresh 24, roll-off
    0.001f, depth_discontinuity_radius ceil(0.5 * block), ROI offsets left max(0, minD + numD) + block / 2, right
    max(0, -minD) + block / 2, top = bottom block / 2; ROI = Rect(left, top, w - left - right, h - top - bottom), the
    right view's Rect(w - (x + width), y, width, height).  OURS: an empty ROI is refused.
W3  Discontinuity map of one view on its ROI crop.  RECALLED: float disparities, mean and mean of squares by a
    (2r+1)^2 normalised box filter, dd = max(0, 1 - roll_off * (E[x^2] - E[x]^2)) in float.  OURS: the sums are formed as
    exact integers (any order), each mean is (float)((double)sum * (1.0 / (2r+1)^2)), the border is reflect-101 on the
    crop (cv::borderInterpolate: a crop of one pixel maps every index to 0, a larger one reflects until inside).
W4  Confidence.  RECALLED: the left pixel's disparity points into the right map, |dl + dr| < LRC_thresh keeps
    min(dd_left, dd_right), everything else 0; the map handed out is conf * 255 as float.  OURS: the indexing is in
    absolute image coordinates, xr = x - (dl >> 4) (arithmetic shift), (y, xr) must lie in the right ROI; no special case
    for invalid left pixels; zero outside the ROI.
W5  FGS (fastGlobalSmootherFilter on the ROI).  RECALLED: num_iter 3, attenuation 0.25, lambda_ref = 1.5 * lambda *
    4^(n-1) / (4^n - 1), weights from a table -exp(-k / sigma) of the absolute grey difference (one channel) or
    -exp(-sqrt(k) / sigma) of the summed squared channel differences (three channels), horizontal then vertical
    tridiagonal solve per iteration, lambda_cur *= 0.25.  OURS: exp = svo_exp, the tables are (float) of doubles, lambda_cur
    is (float)lambda_ref, and the float32 operation order of one sweep is exactly `sweep` below.
W6  Output.  RECALLED: with confidence num = FGS(disp * conf), den = FGS(conf), out = saturate_cast<short>(num / (den +
    FLT_EPSILON)) rounded half to even; without, out = FGS(disp) rounded.  OURS: outside the ROI the output is the input
    left disparity; the confidence map without use_confidence is all zero.
"""
from __future__ import annotations

import dataclasses

import numpy as np

import sgbm_numpy as sn
from sift_numpy import svo_exp

f32, f64 = np.float32, np.float64
FLT_EPSILON = f32(1.1920928955078125e-07)
NUM_ITER = 3


@dataclasses.dataclass
class WlsParams:
    lambda_: float = 8000.0
    sigma_color: float = 1.5
    lrc_thresh: int = 24
    depth_discontinuity_radius: int = 4
    roll_off: float = 0.001
    use_confidence: int = 1
    roi_left: int = 100
    roi_right: int = 3
    roi_top: int = 3
    roi_bottom: int = 3


def right_matcher_params(p: sn.Params) -> sn.Params:
    """W1."""
    return sn.Params(min_disparity=-(p.min_disparity + p.num_disparities) + 1, num_disparities=p.num_disparities,
                     block_size=p.block_size, p1=p.p1, p2=p.p2, disp12_max_diff=1000000, pre_filter_cap=p.pre_filter_cap,
                     uniqueness_ratio=0, speckle_window_size=0, speckle_range=0, mode=p.mode)


def default_params(p: sn.Params, **overrides) -> WlsParams:
    """W2."""
    half = p.block_size // 2
    q = WlsParams(depth_discontinuity_radius=(p.block_size + 1) // 2 if p.block_size > 0 else 0,
                  roi_left=max(0, p.min_disparity + p.num_disparities) + half, roi_right=max(0, -p.min_disparity) + half,
                  roi_top=half, roi_bottom=half)
    for k, v in overrides.items():
        assert hasattr(q, k), k
        setattr(q, k, v)
    return q


def roi(p: WlsParams, w: int, h: int):
    """(x, y, width, height) of the left view's ROI; the right view's starts at w - (x + width)."""
    return p.roi_left, p.roi_top, w - p.roi_left - p.roi_right, h - p.roi_top - p.roi_bottom


def reflect101(i: np.ndarray, n: int) -> np.ndarray:
    i = np.asarray(i, np.int64).copy()
    if n == 1:
        return np.zeros_like(i)
    for _ in range(64):
        bad = (i < 0) | (i >= n)
        if not bad.any():
            break
        i = np.where(i < 0, -i, i)
        i = np.where(i >= n, 2 * (n - 1) - i, i)
    return i


def discontinuity(crop: np.ndarray, radius: int, roll_off: float) -> np.ndarray:
    """W3 on one view's ROI crop (int16) -> float32 of the crop's shape."""
    h, w = crop.shape
    v = crop.astype(np.int64)
    k = np.arange(-radius, radius + 1)
    cols = reflect101(np.arange(w)[:, None] + k[None, :], w)   # [w, 2r+1]
    rows = reflect101(np.arange(h)[:, None] + k[None, :], h)
    s1 = v[:, cols].sum(2)
    s2 = (v * v)[:, cols].sum(2)
    s1 = s1[rows, :].sum(1)
    s2 = s2[rows, :].sum(1)
    scale = 1.0 / float((2 * radius + 1) ** 2)
    mean = (s1.astype(f64) * scale).astype(f32)
    meansq = (s2.astype(f64) * scale).astype(f32)
    var = meansq - mean * mean
    return np.maximum(f32(0), f32(1) - f32(roll_off) * var).astype(f32)


def confidence(disp_left: np.ndarray, disp_right: np.ndarray, p: WlsParams) -> np.ndarray:
    """W3 + W4 -> conf (float32, 0..1) on the left ROI."""
    h, w = disp_left.shape
    x0, y0, rw, rh = roi(p, w, h)
    xr0 = w - (x0 + rw)
    dd_l = discontinuity(disp_left[y0:y0 + rh, x0:x0 + rw], p.depth_discontinuity_radius, p.roll_off)
    dd_r = discontinuity(disp_right[y0:y0 + rh, xr0:xr0 + rw], p.depth_discontinuity_radius, p.roll_off)
    dl = disp_left[y0:y0 + rh, x0:x0 + rw].astype(np.int64)
    xr = (x0 + np.arange(rw))[None, :] - (dl >> 4)
    inside = (xr >= xr0) & (xr < xr0 + rw)
    xr_c = np.clip(xr, xr0, xr0 + rw - 1)
    rows = np.arange(rh)[:, None]
    dr = disp_right[y0 + rows, xr_c].astype(np.int64)
    ok = inside & (np.abs(dl + dr) < p.lrc_thresh)
    return np.where(ok, np.minimum(dd_l, dd_r[rows, xr_c - xr0]), f32(0)).astype(f32)


def lut(sigma: float, c: int) -> np.ndarray:
    """W5: the weight table, float32."""
    if c == 1:
        k = np.arange(256, dtype=f64)
        return (-svo_exp(-k / f64(sigma))).astype(f32)
    k = np.arange(3 * 255 * 255 + 1, dtype=f64)
    return (-svo_exp(-np.sqrt(k) / f64(sigma))).astype(f32)


def weights(guide: np.ndarray, sigma: float):
    """W5: Chor / Cvert of a guide crop (h x w or h x w x 3 uint8)."""
    g = guide.astype(np.int64)
    if g.ndim == 3 and g.shape[2] == 1:
        g = g[..., 0]
    h, w = g.shape[:2]
    if g.ndim == 2:
        t = lut(sigma, 1)
        dh, dv = np.abs(g[:, :-1] - g[:, 1:]), np.abs(g[:-1] - g[1:])
    else:
        t = lut(sigma, 3)
        dh, dv = ((g[:, :-1] - g[:, 1:]) ** 2).sum(2), ((g[:-1] - g[1:]) ** 2).sum(2)
    chor, cvert = np.zeros((h, w), f32), np.zeros((h, w), f32)
    chor[:, :-1] = t[dh]
    cvert[:-1] = t[dv]
    return chor, cvert


def sweep(u: np.ndarray, C: np.ndarray, lam, dtype=f32) -> np.ndarray:
    """W5: one tridiagonal sweep along axis 1 of every row of u (lines x n), weights C (same shape, last column 0)."""
    u = np.array(u, dtype)
    C = np.asarray(C, dtype)
    lam, one = dtype(lam), dtype(1)
    n = u.shape[1]
    t = np.zeros_like(u)
    for j in range(n):
        c = lam * C[:, j]
        if j == 0:
            b = one - c                       # a_0 = 0: (1 - 0) - c
            t[:, 0] = c / b
            u[:, 0] = u[:, 0] / b
        else:
            a = lam * C[:, j - 1]
            b = (one - a) - c
            den = b - a * t[:, j - 1]
            t[:, j] = c / den
            u[:, j] = (u[:, j] - a * u[:, j - 1]) / den
    for j in range(n - 2, -1, -1):
        u[:, j] = u[:, j] - t[:, j] * u[:, j + 1]
    return u


def lambda_ref(lam: float) -> np.float32:
    return f32(1.5 * f64(lam) * f64(4.0 ** (NUM_ITER - 1)) / f64(4.0 ** NUM_ITER - 1.0))


def fgs(plane: np.ndarray, chor: np.ndarray, cvert: np.ndarray, lam: float, dtype=f32) -> np.ndarray:
    u = np.array(plane, dtype)
    lam_cur = dtype(lambda_ref(lam))
    for _ in range(NUM_ITER):
        u = sweep(u, chor, lam_cur, dtype)
        u = np.ascontiguousarray(sweep(u.T, cvert.T, lam_cur, dtype).T)
        lam_cur = dtype(lam_cur * dtype(0.25))
    return u


def _round_i16(x: np.ndarray) -> np.ndarray:
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def wls_filter(disp_left: np.ndarray, disp_right, guide: np.ndarray, p: WlsParams, conf_override=None):
    """W3..W6 -> (filtered int16 h x w, confidence float32 h x w = conf * 255, zero outside the ROI)."""
    h, w = disp_left.shape
    x0, y0, rw, rh = roi(p, w, h)
    assert rw > 0 and rh > 0
    chor, cvert = weights(guide[y0:y0 + rh, x0:x0 + rw], p.sigma_color)
    dl = disp_left[y0:y0 + rh, x0:x0 + rw].astype(f32)
    out = disp_left.copy()
    conf_map = np.zeros((h, w), f32)
    if p.use_confidence:
        conf = confidence(disp_left, disp_right, p) if conf_override is None else conf_override.astype(f32)
        num = fgs(dl * conf, chor, cvert, p.lambda_)
        den = fgs(conf, chor, cvert, p.lambda_)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = num / (den + FLT_EPSILON)
        out[y0:y0 + rh, x0:x0 + rw] = _round_i16(q)
        conf_map[y0:y0 + rh, x0:x0 + rw] = conf * f32(255)
    else:
        out[y0:y0 + rh, x0:x0 + rw] = _round_i16(fgs(dl, chor, cvert, p.lambda_))
    return out, conf_map


def sgbm_wls(left: np.ndarray, right: np.ndarray, sp: sn.Params, wp: WlsParams):
    """The whole chain -> (filtered, disp_left, disp_right, confidence)."""
    dl = sn.sgbm(left, right, sp)
    dr = sn.sgbm(right, left, right_matcher_params(sp)) if wp.use_confidence else None
    out, conf = wls_filter(dl, dr, sn.cv_gray(np.asarray(left)), wp)
    return out, dl, dr, conf
