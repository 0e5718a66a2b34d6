"""tests/bm_numpy.py, the arbiter of csrc/bm.hip, checked on the CPU: against a literal four-loop brute force of B2..B8, that every
branch of the recipe is reached by a fixture (read from the ``stages`` dict), the right-matcher and WLS defaults of B11, and the
accuracy on a ray-cast scene."""
import dataclasses

import numpy as np
import pytest

import bm_fixtures as bf
import bm_numpy as bn
import sgbm_numpy as sn
from ros_stereo_slam_amd import synth


def brute_prefilter(img, cap):
    h, w = img.shape
    I = img.astype(int)
    out = np.full((h, w), cap, int)
    y = 0
    while y < h - 1:
        for yy in (y, y + 1):
            above = yy - 1 if yy > 0 else (1 if h > 1 else 0)
            below = yy + 1 if yy < h - 1 else (yy - 1 if h > 1 else yy)
            for x in range(1, w - 1):
                v = (I[above, x + 1] - I[above, x - 1]) + 2 * (I[yy, x + 1] - I[yy, x - 1]) + (I[below, x + 1] - I[below, x - 1])
                out[yy, x] = min(max(v, -cap), cap) + cap
        y += 2
    return out.astype(np.uint8)


def c_div(a, b):
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def brute_bm(left, right, p):
    """B2..B8, one pixel, one disparity, one window term at a time."""
    h, w = left.shape
    L, R = brute_prefilter(left, p.pre_filter_cap).astype(int), brute_prefilter(right, p.pre_filter_cap).astype(int)
    D, minD, r, cap = p.num_disparities, p.min_disparity, p.block_size // 2, p.pre_filter_cap
    F = (minD - 1) << 4
    out = np.full((h, w), F, int)
    lofs, rofs = max(D - 1 + minD, 0), -min(D - 1 + minD, 0)
    width1 = w - rofs - D + 1
    if lofs >= w or rofs >= w or width1 < 1:
        return out.astype(np.int16)
    for y in range(h):
        for x in range(width1):
            if lofs + x >= w:
                continue
            sad = [0] * D
            tsum = 0
            for i in range(-r, r + 1):
                cy = min(max(y + i, 0), h - 1)
                for j in range(-r, r + 1):
                    cl = min(max(lofs + x + j, 0), w - 1)
                    cr = rofs + min(max(x + j, -rofs), width1 - 1)
                    tsum += abs(L[cy, cl] - cap)
                    for d in range(D):
                        sad[d] += abs(L[cy, cl] - R[cy, cr + d])
            if tsum < p.texture_threshold:
                continue
            minsad, mind = sad[0], 0
            for d in range(1, D):
                if sad[d] < minsad:
                    minsad, mind = sad[d], d
            if p.uniqueness_ratio > 0:
                thresh = minsad + c_div(minsad * p.uniqueness_ratio, 100)
                if any(abs(d - mind) > 1 and sad[d] <= thresh for d in range(D)):
                    continue
            ext = [sad[1]] + sad + [sad[D - 2]]
            pp, nn = ext[mind + 2], ext[mind]
            den = pp + nn - 2 * sad[mind] + abs(pp - nn)
            out[y, lofs + x] = ((D - mind - 1 + minD) * 256 + (c_div((pp - nn) * 256, den) if den else 0) + 15) >> 4
    return out.astype(np.int16)


@pytest.mark.parametrize("w,h,block,minD", [(29, 13, 5, 0), (29, 13, 7, -3), (40, 12, 5, 5), (40, 12, 7, 0), (29, 13, 5, -3),
                                            (40, 12, 7, 5)])
def test_restatement_equals_the_brute_force(w, h, block, minD):
    L, R = bf.textured_pair(w, h, 1, shift=3, seed=w + block, flat=False)
    L[2:8, 10:22] = 77   # a flat patch: the texture test rejects inside it
    for tex, ratio in ((10, 15), (0, 0), (300, 40)):
        p = bn.Params(num_disparities=16, block_size=block, min_disparity=minD, texture_threshold=tex, uniqueness_ratio=ratio)
        st = {}
        got, exp = bn.bm(L, R, p, st), brute_bm(L, R, p)
        assert np.array_equal(st["left_pf"], brute_prefilter(L, p.pre_filter_cap))
        assert np.array_equal(got, exp), (p, np.argwhere(got != exp)[:5])
        F = bn.filtered_value(p)
        assert (got != F).any() or tex == 300


def test_prefilter_heights_and_the_odd_last_row():
    rng = np.random.default_rng(3)
    for h in (1, 2, 3, 6, 7):
        img = rng.integers(0, 256, (h, 17), dtype=np.uint8)
        out = bn.prefilter_xsobel(img, 31)
        assert np.array_equal(out, brute_prefilter(img, 31))
        assert (out[:, 0] == 31).all() and (out[:, -1] == 31).all()
        if h % 2:
            assert (out[-1] == 31).all()                      # B2: the fill loop's row
        if h >= 2:
            assert (out[:h - h % 2, 1:-1] != 31).any()
    # reflect-101 above row 0: a vertical edge seen only in row 1 shows in row 0's output
    img = np.zeros((4, 9), np.uint8)
    img[1, 5:] = 10
    assert bn.prefilter_xsobel(img, 31)[0, 4] == 31 + 10 + 10       # rows 1, 0, 1 (a replicated row 0 would give 31 + 10)
    img = np.zeros((4, 9), np.uint8)
    img[2, 5:] = 10
    assert bn.prefilter_xsobel(img, 31)[3, 4] == 31 + 10 + 10       # rows 2, 3, 2 below the last row


def _stages(L, R, **kw):
    st = {}
    p = bn.Params(**kw)
    out = bn.bm(L, R, p, st)
    return p, st, out


def test_texture_branch_and_its_neighbour():
    L, R = bf.textured_pair(90, 40, 1, shift=4, seed=1)
    p, st, out = _stages(L, R, num_disparities=16, block_size=7)
    lofs = bn.geometry(p, 90)[0]
    F = bn.filtered_value(p)
    low = st["tsum"] < p.texture_threshold
    n = min(st["tsum"].shape[1], 90 - lofs)
    assert low.any() and (out[:, lofs:lofs + n][low[:, :n]] == F).all()
    kept_next = low[:, :n - 1] & ~low[:, 1:n] & (out[:, lofs + 1:lofs + n] != F)
    assert kept_next.any()


def test_uniqueness_at_distance_two_and_not_at_one():
    L, R = bf.textured_pair(90, 40, 1, shift=4, seed=1)
    p, st, out = _stages(L, R, num_disparities=16, block_size=7, texture_threshold=0)
    sad, mind = st["sad"], st["mind"]
    minsad = np.take_along_axis(sad, mind[..., None], 2)[..., 0]
    thresh = minsad + sn.c_div(minsad * p.uniqueness_ratio, 100)
    dist = np.abs(np.arange(16)[None, None] - mind[..., None])
    under = sad <= thresh[..., None]
    lofs = bn.geometry(p, 90)[0]
    band = out[:, lofs:lofs + sad.shape[1]]
    F = bn.filtered_value(p)
    only_two = (under & (dist == 2)).any(2) & ~(under & (dist > 2)).any(2)
    assert only_two.any() and (band[only_two] == F).all()
    only_one = (under & (dist == 1)).any(2) & ~(under & (dist > 1)).any(2)
    assert only_one.any() and (band[only_one] != F).all()


def test_ties_go_to_the_larger_disparity_and_a_zero_denominator():
    L = np.full((12, 40), 50, np.uint8)
    for minD in (-3, 0, 5):
        p, st, out = _stages(L, L, num_disparities=16, block_size=5, min_disparity=minD, texture_threshold=0, uniqueness_ratio=0)
        assert (st["sad"] == 0).all() and (st["mind"] == 0).all()          # every d ties; the first internal index wins
        lofs, _, width1 = bn.geometry(p, 40)
        n = min(width1, 40 - lofs)
        assert (out[:, lofs:lofs + n] == (15 + minD) * 16).all()          # the largest real disparity, den == 0: no fraction
        assert (out[:, :lofs] == bn.filtered_value(p)).all()


def test_winner_at_both_ends_of_the_range():
    for shift, mind_exp in ((15, 0), (0, 15)):
        L, R = bf.textured_pair(70, 16, 1, shift=shift, seed=5, flat=False)
        p, st, out = _stages(L, R, num_disparities=16, block_size=5, uniqueness_ratio=0, texture_threshold=0)
        hit = st["mind"] == mind_exp
        assert hit.mean() > 0.5
        sad = st["sad"]
        y, x = np.argwhere(hit)[len(np.argwhere(hit)) // 2]
        s = sad[y, x]
        pp = s[1] if mind_exp == 0 else s[14]        # sad[ndisp] = sad[ndisp - 2]
        nn = s[1] if mind_exp == 0 else s[14]        # sad[-1] = sad[1]
        den = pp + nn - 2 * s[mind_exp] + abs(pp - nn)
        exp = ((16 - mind_exp - 1) * 256 + (c_div((pp - nn) * 256, den) if den else 0) + 15) >> 4
        assert out[y, bn.geometry(p, 70)[0] + x] == exp == (15 - mind_exp) * 16


def test_an_empty_band_is_all_filtered():
    L, R = bf.textured_pair(20, 8, 1, shift=1, seed=2, flat=False)
    for kw in (dict(num_disparities=32), dict(num_disparities=16, min_disparity=6), dict(num_disparities=16, min_disparity=-40)):
        p = bn.Params(block_size=5, **kw)
        assert bn.empty_band(p, 20) and (bn.bm(L, R, p) == bn.filtered_value(p)).all()
    p = bn.Params(block_size=5, num_disparities=16)           # width1 = 1: one band column
    assert bn.geometry(p, 16) == (15, 0, 1) and not bn.empty_band(p, 16)


def test_validate_disparity_rejects_and_breaks_ties_to_the_left():
    L, R = bf.textured_pair(90, 40, 1, shift=4, seed=1)
    p, st, out = _stages(L, R, num_disparities=16, block_size=7, disp12_max_diff=0, uniqueness_ratio=0, texture_threshold=0)
    assert st["validate_info"]["rejected"] > 0 and (st["validated"] != st["raw"]).sum() == st["validate_info"]["rejected"]
    # a tie in cost2: two left pixels of equal cost on one right column; the leftmost keeps the entry
    disp = np.full((1, 12), -16, np.int16)
    cost = np.zeros((1, 12), np.int32)
    q = bn.Params(num_disparities=16, min_disparity=-15, disp12_max_diff=0)      # minX1 = 1, maxX1 = 12 - 15 < 1: widen
    q = dataclasses.replace(q, min_disparity=-8, num_disparities=16)             # band [8, 4): still empty; use w = 30
    disp = np.full((1, 30), bn.filtered_value(q), np.int16)
    cost = np.zeros((1, 30), np.int32)
    disp[0, 10], disp[0, 12] = 0, 32          # both land on x2 = 10 with cost 7
    cost[0, 10] = cost[0, 12] = 7
    info = {}
    out2 = bn.validate_disparity(disp, cost, q, info)
    assert info["ties"] == 1
    # pixel 12 (d = 2) looks at disp2[10] = 0 (pixel 10's, the leftmost): differs by 32 > 0 -> rejected; pixel 10 agrees with itself
    assert out2[0, 12] == bn.filtered_value(q) and out2[0, 10] == 0 and info["rejected"] == 1
    cost[0, 10] = 8                            # now pixel 12 owns the entry and survives, pixel 10 goes
    out3 = bn.validate_disparity(disp, cost, q)
    assert out3[0, 12] == 32 and out3[0, 10] == bn.filtered_value(q)


def test_speckle_window_is_inclusive():
    from scipy import ndimage

    L, R = bf.textured_pair(120, 48, 1, shift=4, seed=3)
    # a harsh uniqueness ratio leaves islands of a few pixels
    p, st, out = _stages(L, R, num_disparities=16, block_size=5, uniqueness_ratio=150, speckle_window_size=2, speckle_range=1000)
    F = bn.filtered_value(p)
    lab, n = ndimage.label(st["validated"] != F)          # range 1000: every valid 4-neighbour pair is joined
    size = np.bincount(lab.ravel())
    assert (size[1:] == 2).any() and (size[1:] == 3).any()
    small = (size[lab] <= 2) & (lab > 0)
    assert (out[small] == F).all() and np.array_equal(out[~small], st["validated"][~small])
    assert (out[(size[lab] == 3) & (lab > 0)] != F).all()
    p0 = dataclasses.replace(p, speckle_range=-1)          # B10: a negative range switches the filter off
    assert np.array_equal(bn.bm(L, R, p0), st["validated"])


def test_right_matcher_and_wls_defaults():
    p = bn.Params(min_disparity=1, num_disparities=96, speckle_window_size=3000, speckle_range=5, disp12_max_diff=2)
    r = bn.right_matcher_params(p)
    assert dataclasses.asdict(r) == dict(pre_filter_type=1, pre_filter_size=9, pre_filter_cap=31, block_size=21, min_disparity=-96,
                                         num_disparities=96, texture_threshold=0, uniqueness_ratio=0, speckle_window_size=0,
                                         speckle_range=0, disp12_max_diff=1000000)
    wp = bn.wls_default_params(p)
    assert (wp.lambda_, wp.sigma_color, wp.lrc_thresh, wp.roll_off, wp.use_confidence) == (8000.0, 1.5, 24, 0.001, 1)
    assert (wp.depth_discontinuity_radius, wp.roi_left, wp.roi_right, wp.roi_top, wp.roi_bottom) == (7, 107, 10, 10, 10)
    import math
    for b in range(5, 256, 2):
        assert bn.wls_default_params(bn.Params(block_size=b)).depth_discontinuity_radius == math.ceil(0.33 * b)
    d = bn.Params()
    assert dataclasses.astuple(d) == (1, 9, 31, 21, 0, 64, 10, 15, 0, 0, -1)


# measured with the restatement (half-size KITTI geometry, minD 1, D = 48, block 15): 96.22 % within 1 px, 2.85 % FILTERED, of
# 99150 pixels.  The floor: that figure rounded down to a whole per cent, minus one
ACCURACY_FLOOR = 0.95


def scene_accuracy():
    sc = synth.Scene()
    fx, fy, cx, cy = (v / 2 for v in synth.KITTI_K)
    w, h = 620, 188
    left, right, _ = sc.stereo(np.eye(3), np.zeros(3), K=(fx, fy, cx, cy), size=(w, h), channels=1)
    left, right = np.squeeze(left), np.squeeze(right)
    uu, vv = np.meshgrid(np.arange(w, dtype=float), np.arange(h, dtype=float))
    dx, dy = (uu - cx) / fx, (vv - cy) / fy
    with np.errstate(divide="ignore", invalid="ignore"):
        Z = np.where(dy > 1e-9, sc.ground_y / dy, np.inf)
        for xw in (-sc.wall_x, sc.wall_x):
            zz = xw / dx
            ok = (np.abs(dx) > 1e-9) & (zz > 1e-6) & (zz * dy < sc.ground_y) & (zz * dy > sc.ground_y - 8.0)
            Z = np.minimum(Z, np.where(ok, zz, np.inf))
        gt = fx * synth.KITTI_BASELINE / Z
    p = bn.Params(min_disparity=1, num_disparities=48, block_size=15)
    st = {}
    d = bn.bm(left, right, p, st)
    lofs, _, width1 = bn.geometry(p, w)
    textured = np.zeros((h, w), bool)
    textured[:, lofs:lofs + min(width1, w - lofs)] = (st["tsum"] >= p.texture_threshold)[:, :w - lofs]
    m = np.isfinite(Z) & textured & (gt >= 1) & (gt < 47)
    valid = d[m] != bn.filtered_value(p)
    good = valid & (np.abs(d[m] / 16.0 - gt[m]) <= 1.0)
    return good.mean(), 1.0 - valid.mean(), int(m.sum())


def test_accuracy_on_a_ray_cast_scene():
    """Ground truth fx B / Z from the scene's planes at identity pose, re-derived here.  The share of textured in-band pixels that
    are valid and within 1 px of it, measured with the restatement: 96.22 % (ACCURACY_FLOOR above); the floor is
    that figure rounded down to a whole per cent, minus one.  At most 10 % of those pixels may be FILTERED."""
    good, filtered, n = scene_accuracy()
    print(f"bm accuracy: {good:.4f} within 1 px, {filtered:.4f} filtered, {n} pixels")
    assert n > 20000
    assert filtered <= 0.10, filtered
    assert good >= ACCURACY_FLOOR, good
