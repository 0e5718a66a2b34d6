"""A numpy restatement of OpenCV's block-matching stereo matcher, ``cv::StereoBM`` (``StereoBM::create(0, 21)`` +
``compute(left, right, disp)``), its right matcher and the WLS filter's defaults for it (ximgproc ``createRightMatcher`` /
``createDisparityWLSFilter``, BM case).  It is the checker of csrc/bm.hip: every GPU test compares the device result with it
bit for bit, and with nothing else.

OpenCV version assumed: 3.2.  Neither OpenCV nor its sources are available to this project, so what follows is restated from
recollection of modules/calib3d/src/stereobm.cpp (``prefilterXSobel``, ``findStereoCorrespondenceBM``, ``StereoBMImpl::compute``)
and stereosgbm.cpp (``validateDisparity``, ``filterSpeckles``), not copied.  This header is the definition; DESIGN.md section
10q keeps the same list.  Each point is marked "recalled, firm", "recalled, unsure" or "OURS" (decided here).

 B1  recalled, firm.  Parameters and defaults of ``StereoBM::create(0, 21)``: preFilterType XSOBEL, preFilterSize 9,
     preFilterCap 31, blockSize 21, minDisparity 0, numDisparities 64 (what 0 reads as), textureThreshold 10,
     uniquenessRatio 15, speckleWindowSize 0, speckleRange 0, disp12MaxDiff -1.  Output int16, disparity x 16,
     ``FILTERED = (minD - 1) << 4``.  OURS: BGR input is converted with the library's ``cv_gray`` recipe first, as
     ``svo_sgbm_compute`` does (upstream takes grey only).
 B2  XSOBEL pre-filter, ``ftzero = preFilterCap``, ``tab(v) = clamp(v, -ftzero, ftzero) + ftzero``;
     ``out(y, x) = tab((a[x+1] - a[x-1]) + 2 (b[x+1] - b[x-1]) + (c[x+1] - c[x-1]))`` with a, b, c the rows y-1, y, y+1;
     columns 0 and w-1 are ``ftzero``.  recalled, firm: the row above row 0 is row 1 (row 0 when h = 1), the row below the
     last row is the row above it (the loop's ``srow0`` / ``srow3`` choices).  recalled, unsure: rows are produced in pairs
     (y, y+1) for even y < h - 1 and a fill loop writes ``ftzero`` into whatever is left, so AN ODD HEIGHT LEAVES ITS LAST
     ROW ENTIRELY ``ftzero`` (and a 1-row image is all ``ftzero``).  The issue that asked for this file recalls the same
     loop; nothing firmer is available.
 B3  recalled, firm.  ``lofs = max(ndisp - 1 + minD, 0)``, ``rofs = -min(ndisp - 1 + minD, 0)``,
     ``width1 = w - rofs - ndisp + 1``; if ``lofs >= w``, ``rofs >= w`` or ``width1 < 1`` the whole map is FILTERED.
     Columns outside ``[lofs, lofs + width1)`` are FILTERED; every row is computed.  OURS: for minD > 0 that band ends at
     ``w + minD``, past the image; band columns with ``lofs + x >= w`` have no pixel and are computed nowhere.
 B4  recalled, unsure (the clamps restate what upstream's running sums do at the borders).  For band column x in
     [0, width1), row y, internal index d in [0, ndisp) -- real disparity ``ndisp - 1 - d + minD`` --
     ``sad = sum over i, j in [-r, r], r = blockSize / 2, of |L'(cy, cl) - R'(cy, cr)|`` with
     ``cy = clamp(y + i, 0, h - 1)``, ``cl = clamp(lofs + x + j, 0, w - 1)``,
     ``cr = rofs + clamp(x + j, -rofs, width1 - 1) + d``.
 B5  recalled, firm.  ``tsum`` = the same window sum of ``|L'(cy, cl) - ftzero|``; ``tsum < textureThreshold`` -> FILTERED.
 B6  recalled, firm.  Winner: the first internal d with the smallest SAD (strict <), i.e. the largest real disparity on ties.
 B7  recalled, firm.  Uniqueness, when ``uniquenessRatio > 0``: ``thresh = minsad + minsad * ratio / 100`` (C integer
     division); FILTERED if any d with ``|d - mind| > 1`` has ``sad[d] <= thresh``.
 B8  recalled, firm.  Sub-pixel: ``sad[-1] = sad[1]``, ``sad[ndisp] = sad[ndisp - 2]``; ``p = sad[mind + 1]``,
     ``n = sad[mind - 1]``, ``den = p + n - 2 sad[mind] + |p - n|``; the value is
     ``((ndisp - mind - 1 + minD) * 256 + (den != 0 ? (p - n) * 256 / den : 0) + 15) >> 4`` (C division, arithmetic >>).
 B9  recalled, unsure.  ``disp12MaxDiff >= 0`` runs ``validateDisparity(disp, minsad, minD, ndisp, disp12MaxDiff)`` per row:
     ``minX1 = max(minD + ndisp, 0)``, ``maxX1 = w + min(minD, 0)`` (SGBM's band, one column short of B3's on the left);
     ``disp2`` starts at FILTERED and ``cost2`` at INT_MAX; for x from minX1 to maxX1 - 1, a pixel that is not FILTERED has
     ``x2 = x - ((d + 8) >> 4)`` and takes the entry when ``cost2[x2] > c`` (strict: the leftmost pixel wins ties), storing
     its scaled d; then a pixel that is not FILTERED, with ``d0 = d >> 4``, ``d1 = (d + 15) >> 4``, is FILTERED only when
     BOTH ``x - d0`` and ``x - d1`` are inside the image, both disp2 entries are ``> FILTERED`` and both differ from d (the
     scaled value) by more than ``16 * disp12MaxDiff``.  OURS: an ``x2`` outside the image updates nothing (upstream does not
     test; no legal parameter set was found that produces one).
 B10 recalled, firm.  When ``speckleWindowSize > 0`` and ``speckleRange >= 0``:
     ``filterSpeckles(disp, FILTERED, window, 16 * range)`` -- R13 of sgbm_numpy, reused.  There is no median.
 B11 recalled, firm.  createRightMatcher, BM case: ``minDisparity = -(minD + ndisp) + 1``, the same numDisparities,
     blockSize and pre-filter fields, textureThreshold 0, uniquenessRatio 0, disp12MaxDiff 1000000, speckleWindowSize 0
     (OURS: speckleRange 0 with it); run as ``compute(RIGHT, LEFT)``.  createDisparityWLSFilter, BM case: W2 of
     wls_numpy.py with ``depth_discontinuity_radius = ceil(0.33 * blockSize)`` (OURS: formed exactly, as
     ``(33 * blockSize + 99) // 100``); the ROI from this matcher's range and block as W2 forms it.

Left out (refused by the C ABI): PREFILTER_NORMALIZED_RESPONSE, roi1 / roi2, CV_32F output.
"""
from __future__ import annotations

import dataclasses

import numpy as np

import sgbm_numpy as sn
import wls_numpy as wn

PREFILTER_NORMALIZED_RESPONSE, PREFILTER_XSOBEL = 0, 1
INT_MAX = 2 ** 31 - 1


@dataclasses.dataclass
class Params:
    """B1."""
    pre_filter_type: int = PREFILTER_XSOBEL
    pre_filter_size: int = 9
    pre_filter_cap: int = 31
    block_size: int = 21
    min_disparity: int = 0
    num_disparities: int = 64
    texture_threshold: int = 10
    uniqueness_ratio: int = 15
    speckle_window_size: int = 0
    speckle_range: int = 0
    disp12_max_diff: int = -1


def filtered_value(p: Params) -> int:
    return (p.min_disparity - 1) * 16


def prefilter_xsobel(img: np.ndarray, cap: int) -> np.ndarray:
    """B2: uint8 h x w."""
    I = np.asarray(img).astype(np.int32)
    h, w = I.shape
    out = np.full((h, w), cap, np.int32)
    rows = h - (h & 1)   # the pair loop's rows; an odd height's last row stays ftzero
    if rows and w > 2:
        y = np.arange(rows)
        above = np.where(y > 0, y - 1, 1 if h > 1 else 0)
        below = np.where(y < h - 1, y + 1, y - 1 if h > 1 else y)
        a, b, c = I[above], I[y], I[below]
        v = (a[:, 2:] - a[:, :-2]) + 2 * (b[:, 2:] - b[:, :-2]) + (c[:, 2:] - c[:, :-2])
        out[:rows, 1:-1] = np.clip(v, -cap, cap) + cap
    return out.astype(np.uint8)


def geometry(p: Params, w: int):
    """B3: (lofs, rofs, width1)."""
    e = p.num_disparities - 1 + p.min_disparity
    lofs, rofs = max(e, 0), -min(e, 0)
    return lofs, rofs, w - rofs - p.num_disparities + 1


def empty_band(p: Params, w: int) -> bool:
    lofs, rofs, width1 = geometry(p, w)
    return lofs >= w or rofs >= w or width1 < 1


def sad_volume(Lp: np.ndarray, Rp: np.ndarray, p: Params):
    """B4, B5: (sad [h, width1, D], tsum [h, width1]) as int64: the full volume.  A window term depends on (cy, x + j, d)
    only, so the terms are formed once per (row, u = x + j, d) and summed over i, then over j: plain sums, nothing running."""
    h, w = Lp.shape
    D, r, cap = p.num_disparities, p.block_size // 2, p.pre_filter_cap
    lofs, rofs, width1 = geometry(p, w)
    L, R = Lp.astype(np.int64), Rp.astype(np.int64)
    u, d = np.arange(-r, width1 + r), np.arange(D)
    cl = np.clip(lofs + u, 0, w - 1)
    cr = (rofs + np.clip(u, -rofs, width1 - 1))[:, None] + d[None, :]
    lv = L[:, cl]
    term = np.abs(lv[:, :, None] - R[:, cr])           # [h, width1 + 2r, D]
    tterm = np.abs(lv - cap)
    col = np.zeros_like(term)
    tcol = np.zeros_like(tterm)
    for i in range(-r, r + 1):
        cy = np.clip(np.arange(h) + i, 0, h - 1)
        col += term[cy]
        tcol += tterm[cy]
    sad = np.zeros((h, width1, D), np.int64)
    tsum = np.zeros((h, width1), np.int64)
    for j in range(2 * r + 1):                          # u = x + j - r
        sad += col[:, j:j + width1]
        tsum += tcol[:, j:j + width1]
    return sad, tsum


def match(sad: np.ndarray, tsum: np.ndarray, p: Params, w: int):
    """B5-B8 on the volume -> (raw int16 h x w, mind [h, width1], minsad int32 h x w (0 outside the band))."""
    h, width1, D = sad.shape
    minD, F = p.min_disparity, filtered_value(p)
    lofs = geometry(p, w)[0]
    mind = sad.argmin(2)                       # the first smallest
    minsad = np.take_along_axis(sad, mind[..., None], 2)[..., 0]
    ok = tsum >= p.texture_threshold
    if p.uniqueness_ratio > 0:
        thresh = minsad + sn.c_div(minsad * p.uniqueness_ratio, 100)
        far = np.abs(np.arange(D)[None, None, :] - mind[..., None]) > 1
        ok &= ~((sad <= thresh[..., None]) & far).any(2)
    up = np.where(mind + 1 < D, mind + 1, D - 2)       # sad[ndisp] = sad[ndisp - 2]
    dn = np.where(mind - 1 >= 0, mind - 1, 1)          # sad[-1] = sad[1]
    pp = np.take_along_axis(sad, up[..., None], 2)[..., 0]
    nn = np.take_along_axis(sad, dn[..., None], 2)[..., 0]
    den = pp + nn - 2 * minsad + np.abs(pp - nn)
    frac = np.where(den != 0, sn.c_div((pp - nn) * 256, np.where(den != 0, den, 1)), 0)
    val = ((D - mind - 1 + minD) * 256 + frac + 15) >> 4
    raw = np.full((h, w), F, np.int64)
    cost = np.zeros((h, w), np.int64)
    n = max(min(width1, w - lofs), 0)          # B3: band columns that have a pixel
    raw[:, lofs:lofs + n] = np.where(ok, val, F)[:, :n]
    cost[:, lofs:lofs + n] = minsad[:, :n]
    return raw.astype(np.int16), mind, cost.astype(np.int32)


def validate_disparity(disp: np.ndarray, cost: np.ndarray, p: Params, info: dict | None = None) -> np.ndarray:
    """B9.  info (optional) collects 'ties' (x2 entries met with an equal cost) and 'rejected' (pixel count)."""
    h, w = disp.shape
    minD, maxD, F = p.min_disparity, p.min_disparity + p.num_disparities, filtered_value(p)
    minX1, maxX1 = max(maxD, 0), w + min(minD, 0)
    lim = 16 * p.disp12_max_diff
    out = disp.astype(np.int64)
    ties = rejected = 0
    for y in range(h):
        row = out[y]
        disp2 = np.full(w, F, np.int64)
        cost2 = np.full(w, INT_MAX, np.int64)
        for x in range(minX1, maxX1):
            d = row[x]
            if d == F:
                continue
            x2 = x - ((d + 8) >> 4)
            if not 0 <= x2 < w:
                continue
            c = cost[y, x]
            ties += cost2[x2] == c
            if cost2[x2] > c:
                cost2[x2], disp2[x2] = c, d
        for x in range(minX1, maxX1):
            d = row[x]
            if d == F:
                continue
            x0, x1 = x - (d >> 4), x - ((d + 15) >> 4)
            if (0 <= x0 < w and disp2[x0] > F and abs(disp2[x0] - d) > lim and
                    0 <= x1 < w and disp2[x1] > F and abs(disp2[x1] - d) > lim):
                row[x] = F
                rejected += 1
    if info is not None:
        info.update(ties=int(ties), rejected=int(rejected))
    return out.astype(np.int16)


def bm(left: np.ndarray, right: np.ndarray, p: Params | None = None, stages: dict | None = None) -> np.ndarray:
    """StereoBM::compute(left, right) -> int16 h x w (disparity x 16).  BGR or grey uint8 inputs."""
    p = p or Params()
    gl, gr = sn.cv_gray(np.asarray(left)), sn.cv_gray(np.asarray(right))
    h, w = gl.shape
    Lp, Rp = prefilter_xsobel(gl, p.pre_filter_cap), prefilter_xsobel(gr, p.pre_filter_cap)
    if stages is not None:
        stages.update(left_pf=Lp, right_pf=Rp)
    if empty_band(p, w):
        disp = np.full((h, w), filtered_value(p), np.int16)
        if stages is not None:
            stages.update(sad=None, tsum=None, mind=None, raw=disp.copy(), final=disp.copy())
        return disp
    sad, tsum = sad_volume(Lp, Rp, p)
    raw, mind, cost = match(sad, tsum, p, w)
    disp = raw
    info = {}
    if p.disp12_max_diff >= 0:
        disp = validate_disparity(disp, cost, p, info)
    validated = disp
    if p.speckle_window_size > 0 and p.speckle_range >= 0:
        disp = sn.filter_speckles(disp, filtered_value(p), p.speckle_window_size, 16 * p.speckle_range)
    if stages is not None:
        stages.update(sad=sad, tsum=tsum, mind=mind, minsad=cost, raw=raw.copy(), validated=validated.copy(), validate_info=info,
                      final=disp.copy())
    return disp


def right_matcher_params(p: Params) -> Params:
    """B11."""
    return dataclasses.replace(p, min_disparity=-(p.min_disparity + p.num_disparities) + 1, texture_threshold=0,
                               uniqueness_ratio=0, disp12_max_diff=1000000, speckle_window_size=0, speckle_range=0)


def wls_default_params(p: Params, **overrides) -> wn.WlsParams:
    """B11: W2 with the BM radius."""
    half = p.block_size // 2
    q = wn.WlsParams(depth_discontinuity_radius=(33 * p.block_size + 99) // 100 if p.block_size > 0 else 0,
                     roi_left=max(0, p.min_disparity + p.num_disparities) + half, roi_right=max(0, -p.min_disparity) + half,
                     roi_top=half, roi_bottom=half)
    for k, v in overrides.items():
        assert hasattr(q, k), k
        setattr(q, k, v)
    return q


def bm_wls(left, right, p: Params | None = None, wls: wn.WlsParams | None = None):
    """The chain svo_bm_wls_compute runs: (filtered, disp_left, disp_right, confidence)."""
    p = p or Params()
    wls = wls or wls_default_params(p)
    dl = bm(left, right, p)
    dr = bm(right, left, right_matcher_params(p))
    out, conf = wn.wls_filter(dl, dr, sn.cv_gray(np.asarray(left)), wls)
    return out, dl, dr, conf
