"""Oracle of the loop detector's feature extractor (oracle/orb.c, standing in for cv::ORB at
src/optimizationStuff.cpp:49-56) against independent numpy/scipy restatements of its parts and
the properties that make it usable: repeatable keypoints, rotation-steered descriptors."""
import numpy as np
import pytest
from scipy import ndimage

from oracle import orc
from ros_stereo_slam_amd import synth


def _scene_image():
    sc = synth.Scene()
    R, t = synth.corridor_trajectory(1)[0]
    return sc.stereo(R, t)[0]


def _hamming(a, b):
    return np.array([[bin(int(w)).count("1") for w in (x ^ y)] for x, y in zip(a, b)]).sum(axis=1)


def test_gray_blur_harris_fast_parts():
    img = _scene_image()
    g = orc.bgr_to_gray(img)
    i64 = img.astype(np.int64)
    ref = ((1868 * i64[..., 0] + 9617 * i64[..., 1] + 4899 * i64[..., 2] + 8192) >> 14).astype(np.uint8)
    assert np.array_equal(g, ref)
    k = np.outer([1, 4, 6, 4, 1], [1, 4, 6, 4, 1])
    ref = (ndimage.correlate(g.astype(np.int64), k, mode="mirror") + 128) >> 8
    assert np.array_equal(orc.blur5(g), ref.astype(np.uint8))
    # Harris at a few pixels against the formula with numpy integer sums
    gi = g.astype(np.int64)
    for (x, y) in [(100, 80), (640, 200), (33, 25), (1200, 350)]:
        a = b = c = 0
        for j in range(-3, 4):
            for i in range(-3, 4):
                yy, xx = y + j, x + i
                ix = (gi[yy, xx + 1] - gi[yy, xx - 1]) * 2 + (gi[yy - 1, xx + 1] - gi[yy - 1, xx - 1]) + (gi[yy + 1, xx + 1] - gi[yy + 1, xx - 1])
                iy = (gi[yy + 1, xx] - gi[yy - 1, xx]) * 2 + (gi[yy + 1, xx - 1] - gi[yy - 1, xx - 1]) + (gi[yy + 1, xx + 1] - gi[yy - 1, xx + 1])
                a, b, c = a + ix * ix, b + iy * iy, c + ix * iy
        fa, fb, fc = np.float32(a), np.float32(b), np.float32(c)
        sc = np.float32(1.0) / np.float32(4 * 7 * 255.0)
        s4 = sc * sc * sc * sc
        ref = (fa * fb - fc * fc - np.float32(0.04) * (fa + fb) * (fa + fb)) * s4
        assert orc.harris(g, x, y) == np.float32(ref)
    # FAST-9: a bright quadrant corner fires, a flat patch and a straight edge do not
    t = np.full((40, 40), 50, np.uint8)
    assert not orc.fast9(t, 20, 20)
    e = t.copy(); e[:, 20:] = 200
    assert not orc.fast9(e, 20, 20)
    c = t.copy(); c[20:, 20:] = 200
    assert orc.fast9(c, 20, 20) or orc.fast9(c, 21, 21) or orc.fast9(c, 19, 19)
    pat = orc.orb_pattern()
    assert np.abs(pat).max() <= 13 and not np.any((pat[:, 0] == pat[:, 2]) & (pat[:, 1] == pat[:, 3]))
    assert len({tuple(r) for r in pat}) > 250      # the tests are (almost) all distinct


def test_extract_budget_order_and_margins():
    img = _scene_image()
    xy, octv, resp, d, desc = orc.orb_extract(img, 500)
    assert 300 < len(xy) <= 500
    assert set(np.unique(octv)) <= {0, 1, 2} and np.all(np.diff(octv) >= 0)
    for l in range(3):
        m = octv == l
        lx, ly = xy[m, 0] / 2 ** l, xy[m, 1] / 2 ** l
        w, h = (1241 + (1 << l) - 1) >> l, (376 + (1 << l) - 1) >> l
        assert np.all((lx >= 19) & (lx < w - 19) & (ly >= 19) & (ly < h - 19))
        assert np.all(np.diff(ly * 10000 + lx) > 0)              # raster order inside an octave
    assert np.allclose(np.linalg.norm(d, axis=1), 1, atol=1e-6)
    bits = np.unpackbits(desc.view(np.uint8), axis=1)
    assert 0.3 < bits.mean() < 0.7                                # balanced tests


def test_descriptors_follow_rotation_and_keypoints_repeat():
    img = _scene_image()
    g = orc.bgr_to_gray(img)[:, 200:576]                          # a square crop: 376 x 376
    xa, oa, ra, da, desc_a = orc.orb_extract(g, 300)
    rot = np.ascontiguousarray(np.rot90(g))                       # 90 degrees counter-clockwise
    xb, ob, rb, db, desc_b = orc.orb_extract(rot, 300)
    # (x, y) -> (y, W-1-x) under rot90; match level-0 keypoints by position
    a0, b0 = xa[oa == 0], xb[ob == 0]
    mapped = np.c_[a0[:, 1], 375 - a0[:, 0]]
    pairs = [(i, int(np.argmin(np.abs(b0 - m).sum(axis=1)))) for i, m in enumerate(mapped)]
    pairs = [(i, j) for i, j in pairs if np.abs(b0[j] - mapped[i]).sum() == 0]
    assert len(pairs) > 0.6 * len(a0)                             # the detector is (mostly) rotation covariant
    ia = np.flatnonzero(oa == 0)[[p[0] for p in pairs]]
    ib = np.flatnonzero(ob == 0)[[p[1] for p in pairs]]
    dist = _hamming(desc_a[ia], desc_b[ib])
    assert np.median(dist) < 40                                   # steered tests see (nearly) the same pixels
    rnd = _hamming(desc_a[ia], desc_b[np.roll(ib, 7)])
    assert np.median(rnd) > 90                                    # unrelated descriptors are far apart


# ---- cv::ORB's own shape (oracle/orb.c: orc_orb_extract_cv), its parts against independent restatements ----
def test_cv_levels_and_quota_follow_upstreams_formulas():
    ws, hs, sc, q = orc.orb_cv_levels(1241, 376, 8, 1.2, 500)
    assert list(ws) == [1241, 1034, 862, 718, 598, 499, 416, 346] and list(hs) == [376, 313, 261, 218, 181, 151, 126, 105]
    assert np.allclose(sc, 1.2 ** np.arange(8), rtol=1e-6)
    # n (1 - f) / (1 - f^8), scaled by f per level, rounded; the last level takes the rest
    f = np.float32(1.0 / 1.2)
    want = np.float32(500) * (1 - f) / (1 - np.float32(float(f) ** 8))
    exp, tot = [], 0
    for _ in range(7):
        exp.append(int(np.rint(want)))
        tot += exp[-1]
        want = np.float32(want * f)
    exp.append(500 - tot)
    assert list(q) == exp and q.sum() == 500


def test_cv_resize_is_bilinear_in_11_bit_fixed_point():
    rng = np.random.default_rng(2)
    g = ndimage.gaussian_filter(rng.integers(0, 256, (97, 131)).astype(np.float64), 1.5)
    g = np.clip(g, 0, 255).astype(np.uint8)
    dw, dh = 109, 81
    out = orc.resize_linear(g, dw, dh)
    # float bilinear at the pixel-centre mapping: the fixed-point result is within one grey level
    sx, sy = g.shape[1] / dw, g.shape[0] / dh
    X = np.clip((np.arange(dw) + 0.5) * sx - 0.5, 0, g.shape[1] - 1)
    Y = np.clip((np.arange(dh) + 0.5) * sy - 0.5, 0, g.shape[0] - 1)
    ref = ndimage.map_coordinates(g.astype(np.float64), np.meshgrid(Y, X, indexing="ij"), order=1, mode="nearest")
    assert np.abs(out.astype(np.float64) - ref).max() <= 1.0
    # and exactly the fixed-point recipe as tests/orb_numpy.py restates it (every ratio and odd size: test_orb_numpy.py)
    import orb_numpy

    assert np.array_equal(out, orb_numpy.resize_linear(g, dw, dh))
    assert np.array_equal(orc.resize_linear(g, g.shape[1], g.shape[0]), g)      # the identity map is exact
    flat = np.full((50, 70), 93, np.uint8)
    assert np.all(orc.resize_linear(flat, 58, 42) == 93)


def test_cv_gauss7_kernel_and_rounding():
    rng = np.random.default_rng(5)
    g = rng.integers(0, 256, (60, 80)).astype(np.uint8)
    x = np.arange(-3, 4)
    k = np.exp(-x * x / 8.0)
    k = np.rint(k / k.sum() * 256).astype(np.int64)
    assert list(k) == [18, 34, 49, 55, 49, 34, 18]
    ref = (ndimage.correlate(g.astype(np.int64), np.outer(k, k), mode="mirror") + (1 << 15)) >> 16
    assert np.array_equal(orc.gauss7(g), np.minimum(ref, 255).astype(np.uint8))
    assert np.all(orc.gauss7(np.full((20, 20), 255, np.uint8)) == 255)          # 257 / 256 saturates, as upstream's does


def test_cv_fast_score_is_the_largest_threshold_that_keeps_the_corner():
    img = orc.bgr_to_gray(_scene_image())
    found = 0
    for y in range(40, 330, 3):
        for x in range(40, 1200, 7):
            s = orc.fast_score(img, x, y, 20)
            if s:
                found += 1
                assert s >= 20
                assert orc.fast9(img, x, y, s) and not orc.fast9(img, x, y, s + 1)
            else:
                assert not orc.fast9(img, x, y, 20)
    assert found > 20


def test_cv_fast_atan2_against_numpy():
    rng = np.random.default_rng(7)
    for y, x in rng.normal(0, 1000, (400, 2)):
        ref = np.degrees(np.arctan2(y, x)) % 360.0
        d = abs(orc.fast_atan2(y, x) - ref)
        assert min(d, 360 - d) < 0.02     # upstream states 0.3 degrees; the polynomial is good to ~0.01


def test_cv_extractor_budget_margin_and_rotation_steering():
    img = _scene_image()
    xy, octv, resp, d, ang, desc = orc.orb_extract_cv(img)
    ws, hs, sc, q = orc.orb_cv_levels(img.shape[1], img.shape[0])
    assert len(xy) <= 500 and len(xy) > 300
    counts = np.bincount(octv, minlength=8)
    assert np.all(counts <= q)
    lvl_xy = xy / sc[octv][:, None]
    assert np.all(np.abs(lvl_xy - np.rint(lvl_xy)) < 1e-3)
    assert np.all(np.rint(lvl_xy[:, 0]) >= 31) and np.all(np.rint(lvl_xy[:, 0]) < ws[octv] - 31)
    assert np.all(np.rint(lvl_xy[:, 1]) >= 31) and np.all(np.rint(lvl_xy[:, 1]) < hs[octv] - 31)
    assert np.allclose(d[:, 0], np.cos(np.radians(ang)), atol=1e-6) and np.allclose(d[:, 1], np.sin(np.radians(ang)), atol=1e-6)
    # the image rotated by 180 degrees: the level-0 key points map onto each other, orientations turn by 180, and the
    # steered descriptors stay close (exactly equal up to the asymmetries of the pixel grid)
    rot = np.ascontiguousarray(img[::-1, ::-1])
    xy2, oct2, _, _, ang2, desc2 = orc.orb_extract_cv(rot)
    a0, b0 = xy[octv == 0], xy2[oct2 == 0]
    mapped = np.array([img.shape[1] - 1, img.shape[0] - 1], np.float32) - b0
    hits = 0
    for p, dd, an in zip(a0, desc[octv == 0], ang[octv == 0]):
        j = np.where(np.all(mapped == p, axis=1))[0]
        if len(j):
            hits += 1
            assert abs(((ang2[oct2 == 0][j[0]] - an) % 360) - 180) < 1.0
            assert _hamming(dd[None], desc2[oct2 == 0][j[0]][None])[0] <= 24
    assert hits > 0.8 * len(a0)
    # a settable pattern: other descriptors, the same key points
    pat = orc.orb_pattern()[::-1].copy()
    xy3, _, _, _, _, desc3 = orc.orb_extract_cv(img, pattern=pat)
    assert np.array_equal(xy3, xy) and not np.array_equal(desc3, desc)
