"""The SGBM restatement (tests/sgbm_numpy.py) against things it did not write itself: hand-computed recurrences,
C division, the uniqueness rule, integer-shift pairs, a separately written flood fill, the closed form of Q and the
analytic depth of a ray-cast scene."""
from collections import deque

import numpy as np
import pytest

import sgbm_numpy as sn
from ros_stereo_slam_amd import synth


def test_path_recurrence_by_hand():
    P1, P2 = 2, 10
    Cblock = np.array([[5, 1, 9], [2, 8, 3], [7, 7, 0]])
    C = (Cblock + P2).astype(np.int16)[None]                  # one row, three band pixels, D = 3
    p = sn.Params(p1=P1, p2=P2)
    L = sn.path_costs(C, p, 0)[0]
    # step 1 from Lr' = 0: C itself; step 2: d0 takes Lr'(d+1) + P1 = 3; step 3: d1 takes Lr'(d-1) + P1 = 6
    assert L.tolist() == [[5, 1, 9], [4, 8, 5], [7, 9, 1]]
    # the right -> left direction walks the same line backwards
    assert sn.path_costs(C, p, 4)[0, 2].tolist() == [7, 7, 0]
    # a P2 hit: Lr' = [0, 30, 60] -> d1 from its neighbour (+P1), d2 from minLr' (+P2)
    Lint, L16, m16 = sn.path_step(np.full((1, 3), P2, np.int16), np.array([[0, 30, 60]], np.int16), np.zeros(1, np.int16),
                                  P1, P2)
    assert Lint[0].tolist() == [0, 2, 10] and int(m16[0]) == 0


def test_sweep_sums_the_int_path_costs_not_the_stored_ones():
    """R6 / R7 where Lr leaves int16: one band pixel, P2 = 32000, C = [-1000, 5].  Every path starts here, so each of
    the five L is C + min(0, .., P2) - P2 = [-33000, -31995].  The stored Lr wraps to 32536; the sum takes the int:
    sat16(4 * -33000) = -32768, and sat16(-32768 - 33000) = -32768 (a sum of stored values would give 32767 - 33000)."""
    p = sn.Params(p1=24, p2=32000)
    C = np.array([[[-1000, 5]]], np.int16)
    Lint, L16, m16 = sn.path_step(C[0], np.zeros((1, 2), np.int16), np.zeros(1, np.int16), 24, 32000)
    assert Lint[0].tolist() == [-33000, -31995] and L16[0].tolist() == [32536, -31995] and int(m16[0]) == 32536
    assert sn.aggregate(C, p)[0, 0].tolist() == [-32768, -32768]


def test_prefilter_is_stored_as_uchar_above_cap_127():
    """R1 / R2 by hand on one row (the rows above and below are the row itself: v = 4 (I[x+1] - I[x-1])).
    v = [., 300, 300, -340, 500, 40, 60, -40, .]."""
    row = np.array([[10, 0, 85, 75, 0, 200, 10, 215, 0]], np.uint8)
    inner = [0, 85, 75, 0, 200, 10, 215]
    # cap 127, ftzero 127: nothing wraps; clamp(v) + 127
    der, inten = sn._prefilter_rows(row, max(127, 15) | 1)
    assert der[0].tolist() == [127, 254, 254, 0, 254, 167, 187, 87, 127] and inten[0].tolist() == [127, *inner, 127]
    # cap 200, ftzero 201: +300 clamps to 201 and stores (201 + 201) & 255 = 146; 40 + 201 = 241 fits, 60 + 201 = 261
    # wraps to 5; the border tab[0] = 201 in both channels
    der, inten = sn._prefilter_rows(row, max(200, 15) | 1)
    assert der[0].tolist() == [201, 146, 146, 0, 146, 241, 5, 161, 201] and inten[0].tolist() == [201, *inner, 201]
    # cap 300, ftzero 301: the border stores 301 & 255 = 45; 300 + 301 = 601 -> 89, 301 + 301 = 602 -> 90
    der, inten = sn._prefilter_rows(row, max(300, 15) | 1)
    assert der[0].tolist() == [45, 89, 89, 0, 90, 85, 105, 5, 45] and inten[0].tolist() == [45, *inner, 45]
    # and through pixel_cost: the costs of cap 200 are those of uchar rows, below 256 in the derivative channel
    left, right = np.repeat(row, 3, 0), np.repeat(row[:, ::-1], 3, 0)
    pix = sn.pixel_cost(left, right, sn.Params(min_disparity=0, num_disparities=4, pre_filter_cap=200))
    assert pix.max() <= 255 + (255 >> 2)


def test_c_division_truncates_toward_zero():
    assert sn.c_div(-7, 4) == -1 and sn.c_div(7, 4) == 1 and sn.c_div(-8, 4) == -2 and sn.c_div(-614, 116) == -5


def _wta_one(Srow, **kw):
    """wta() of one band pixel (min_disparity 0, D = len(Srow), image width D + 1)."""
    D = len(Srow)
    p = sn.Params(min_disparity=0, num_disparities=D, **kw)
    S = np.asarray(Srow, np.int64)[None, None, :]
    return int(sn.wta(S, p, D + 1)[0, D])


def test_subpixel_at_a_negative_numerator():
    S = [1000] * 16
    S[2], S[3], S[4] = 58, 50, 100
    # denom2 = 58, numerator (58 - 100) 16 + 58 = -614: -614 / 116 = -5 in C (floor division would give -6)
    assert _wta_one(S) == 3 * 16 - 5
    S[2], S[4] = 100, 58
    assert _wta_one(S) == 3 * 16 + (42 * 16 + 58) // 116


def test_uniqueness_ratio_10():
    S = [1000] * 16
    S[5], S[6] = 100, 101            # a direct neighbour never counts
    S[9] = 112                       # 112 * 90 >= 100 * 100: unique
    assert _wta_one(S, uniqueness_ratio=10) != -16
    S[9] = 105                       # 105 * 90 < 100 * 100 two disparities away: dropped
    assert _wta_one(S, uniqueness_ratio=10) == -16
    assert _wta_one(S, uniqueness_ratio=0) != -16   # ratio 0: a no-op


@pytest.mark.parametrize("block", [1, 3, 5, 7, 11])
@pytest.mark.parametrize("s", [4, 11])
def test_integer_shift_pairs(block, s):
    """left(x) = right(x - s): the rounded disparity is s on at least 95 % of the interior pixels (the sub-pixel term
    is not exactly zero: the BT costs of a band-limited texture are not symmetric about the true match)."""
    w, h = 200, 40
    a, b = synth.textured_pair(w, h, 1, shift=(s, 0))
    p = sn.Params(block_size=block, speckle_window_size=0, num_disparities=32, min_disparity=0)
    d = sn.sgbm(b[..., 0], a[..., 0], p)
    inner = d[6:-6, 32 + 6:-6].astype(np.float64) / 16
    assert np.mean(np.rint(inner) == s) >= 0.95, np.mean(np.rint(inner) == s)


def _flood_fill_reference(d, new_val, max_size, max_diff):
    h, w = d.shape
    out = d.copy()
    seen = np.zeros((h, w), bool)
    for y0 in range(h):
        for x0 in range(w):
            if seen[y0, x0] or d[y0, x0] == new_val:
                continue
            comp, q = [], deque([(y0, x0)])
            seen[y0, x0] = True
            while q:
                y, x = q.popleft()
                comp.append((y, x))
                for yy, xx in ((y + 1, x), (y - 1, x), (y, x + 1), (y, x - 1)):
                    if (0 <= yy < h and 0 <= xx < w and not seen[yy, xx] and d[yy, xx] != new_val
                            and abs(int(d[yy, xx]) - int(d[y, x])) <= max_diff):
                        seen[yy, xx] = True
                        q.append((yy, xx))
            if len(comp) <= max_size:
                for y, x in comp:
                    out[y, x] = new_val
    return out


@pytest.mark.parametrize("seed", range(4))
def test_speckle_filter_matches_a_flood_fill(seed):
    rng = np.random.default_rng(seed)
    h, w = 40, 60
    base = rng.integers(0, 6, (h // 4 + 1, w // 4 + 1)).repeat(4, 0).repeat(4, 1)[:h, :w] * 40
    d = (base + rng.integers(-20, 21, (h, w))).astype(np.int16)
    d[rng.random((h, w)) < 0.1] = 0
    for max_size, max_diff in ((3, 16), (20, 32), (200, 80)):
        assert np.array_equal(sn.filter_speckles(d, 0, max_size, max_diff),
                              _flood_fill_reference(d, 0, max_size, max_diff))


@pytest.mark.parametrize("tx", [0.5707, -0.5707])
def test_q_closed_form(tx):
    fx, fy, cx, cy = 718.856, 718.856, 607.1928, 185.2157
    Q = sn.stereo_rectify_q(fx, fy, cx, cy, tx, 1241, 376)
    want = np.array([[1, 0, 0, -cx], [0, 1, 0, -cy], [0, 0, 0, fy], [0, 0, -1 / tx, 0]])
    assert np.allclose(Q, want, rtol=0, atol=1e-4)   # the principal point passes through float32 corners
    # the reference's t = +baseline: W = -d / baseline, Z = f / W < 0 for every positive disparity
    xyz, _ = sn.reproject(np.full((376, 1241), 16 * 40, np.int16), np.zeros((376, 1241, 3), np.uint8), Q,
                          z_min=-np.inf, z_max=np.inf)
    assert (xyz[:, 2] < 0).all() if tx > 0 else (xyz[:, 2] > 0).all()


def test_reference_window_keeps_nothing_from_valid_pixels():
    Q = sn.stereo_rectify_q(718.856, 718.856, 607.1928, 185.2157, 0.5707, 1241, 376)
    disp = np.random.default_rng(0).integers(0, 97 * 16, (376, 1241)).astype(np.int16)
    xyz, bgr = sn.reproject(disp, np.zeros((376, 1241, 3), np.uint8), Q)
    assert len(xyz) == 0 and len(bgr) == 0


def test_accuracy_on_a_ray_cast_scene():
    """Ground truth fx B / Z from the scene's planes, re-derived here (not read from the renderer).  Measured with the
    restatement: 98.2 % of the textured pixels inside the band within 1 px; the threshold leaves a 3-point margin."""
    sc = synth.Scene()
    left, right, _ = sc.stereo(np.eye(3), np.zeros(3), channels=3)
    fx, fy, cx, cy = synth.KITTI_K
    w, h = synth.KITTI_SIZE
    uu, vv = np.meshgrid(np.arange(w, dtype=float), np.arange(h, dtype=float))
    dx, dy = (uu - cx) / fx, (vv - cy) / fy
    with np.errstate(divide="ignore", invalid="ignore"):
        Z = np.where(dy > 1e-9, sc.ground_y / dy, np.inf)
        for xw in (-sc.wall_x, sc.wall_x):
            zz = xw / dx
            ok = (np.abs(dx) > 1e-9) & (zz > 1e-6) & (zz * dy < sc.ground_y) & (zz * dy > sc.ground_y - 8.0)
            Z = np.minimum(Z, np.where(ok, zz, np.inf))
        gt = fx * synth.KITTI_BASELINE / Z
    d = sn.sgbm(left, right)
    m = np.isfinite(Z) & (uu >= 97) & (gt < 96)
    frac = np.mean(np.abs(d[m] / 16.0 - gt[m]) <= 1.0)
    assert frac >= 0.95, frac
