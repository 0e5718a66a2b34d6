"""The restatement of the disparity WLS filter (tests/wls_numpy.py) held to things outside itself:
the tridiagonal sweep against a dense solve, the smoother's invariants, the closed forms of the discontinuity map, the
left-right check on hand-built maps and the parameter values of the reference's matcher."""
import numpy as np
import pytest

import sgbm_numpy as sn
import wls_numpy as wn

f32, f64 = np.float32, np.float64


def _dense(C, lam):
    n = len(C)
    A = np.zeros((n, n))
    for j in range(n):
        a = lam * C[j - 1] if j else 0.0
        c = lam * C[j]
        A[j, j] = 1.0 - a - c
        if j:
            A[j, j - 1] = a
        if j + 1 < n:
            A[j, j + 1] = c
    return A


@pytest.mark.parametrize("lam", [0.0, 3.0, 400.0 * 1.5 * 16 / 63, 8000.0 * 1.5 * 16 / 63])
@pytest.mark.parametrize("n", [1, 2, 37])
def test_float64_sweep_solves_the_tridiagonal_system(lam, n):
    rng = np.random.default_rng(n)
    C = -rng.uniform(0.0, 1.0, (5, n))
    C[:, -1] = 0.0
    u = rng.uniform(-1500.0, 1500.0, (5, n))
    got = wn.sweep(u, C, lam, dtype=f64)
    for k in range(5):
        want = np.linalg.solve(_dense(C[k], lam), u[k])
        # strictly diagonally dominant, condition <= 1 + 4 lam: float64 leaves this margin
        assert np.abs(got[k] - want).max() <= 1e-9 * max(np.abs(want).max(), 1e-300)


def test_constant_plane_stays_constant():
    rng = np.random.default_rng(2)
    guide = rng.integers(0, 256, (23, 31), dtype=np.uint8)
    chor, cvert = wn.weights(guide, 1.5)
    out = wn.fgs(np.full((23, 31), 777.0, f32), chor, cvert, 8000.0)
    # rows of the system sum to one, so the constant is the exact solution.  In float32 the diagonal 1 - a - c is formed next
    # to |a| + |c| <= 2 lam: a sweep is a solve with a matrix of condition <= 1 + 4 lam perturbed by one rounding, so it
    # moves the constant by at most about (1 + 4 lam) eps relative; two sweeps per iteration, lam = lam_ref, / 4, / 16
    lam = float(wn.lambda_ref(8000.0))
    bound = sum(2 * (1 + 4 * lam / 4 ** k) for k in range(3)) * float(np.finfo(f32).eps)
    assert 1e-3 < bound < 1e-2
    assert np.abs(out / f32(777) - 1).max() < bound


def test_smoothing_does_not_cross_a_step_edge():
    guide = np.zeros((12, 40), np.uint8)
    guide[:, 20:] = 255
    chor, cvert = wn.weights(guide, 0.4)   # exp(-255 / 0.4) = 0 in float: the two halves are decoupled
    assert (chor[:, 19] == 0).all() and (chor[:, :19] == -1).all()
    rng = np.random.default_rng(5)
    plane = (np.where(np.arange(40)[None, :] < 20, 100.0, 900.0) + rng.uniform(-20, 20, (12, 40))).astype(f32)
    lam = 1e4
    out = wn.fgs(plane, chor, cvert, lam)
    other = plane.copy()
    other[:, 20:] = rng.uniform(-3000, 3000, (12, 20))
    assert np.array_equal(wn.fgs(other, chor, cvert, lam)[:, :20], out[:, :20])   # nothing of the right half arrives
    # the exact solve keeps each half's mean (symmetric, unit row sums); float32 moves it by the constant-plane bound
    rel = sum(2 * (1 + 4 * float(wn.lambda_ref(lam)) / 4 ** k) for k in range(3)) * float(np.finfo(f32).eps)
    for half, src in ((out[:, :20], plane[:, :20]), (out[:, 20:], plane[:, 20:])):
        assert abs(half.mean(dtype=f64) - src.mean(dtype=f64)) < rel * 900
        # the slowest mode of 20 columns (eigenvalue 2 - 2 cos(pi / 20)) shrinks by 1 / (1 + lam_cur * 0.0246) per sweep:
        # 40 / 95 / 24 / 6.9 < 0.01, under the float32 error
        assert np.ptp(half) < 2 * rel * 900


def test_unit_confidence_equals_the_plain_path():
    rng = np.random.default_rng(7)
    h, w = 30, 60
    disp = (rng.integers(40, 200, (h, w)) + 30 * (np.arange(w)[None, :] > 30)).astype(np.int16)
    guide = rng.integers(0, 256, (h, w), dtype=np.uint8)
    p = wn.WlsParams(lambda_=400.0, sigma_color=20.0, roi_left=5, roi_right=2, roi_top=1, roi_bottom=3)
    x0, y0, rw, rh = wn.roi(p, w, h)
    with_conf, cmap = wn.wls_filter(disp, None, guide, p, conf_override=np.ones((rh, rw), f32))
    p.use_confidence = 0
    plain, cmap0 = wn.wls_filter(disp, None, guide, p)
    assert np.abs(with_conf.astype(int) - plain.astype(int)).max() <= 1   # up to the final rounding
    assert (with_conf != disp).any()
    assert (cmap[y0:y0 + rh, x0:x0 + rw] == 255).all() and cmap.sum() == 255.0 * rw * rh and not cmap0.any()
    out_roi = np.ones((h, w), bool)
    out_roi[y0:y0 + rh, x0:x0 + rw] = False
    assert np.array_equal(plain[out_roi], disp[out_roi])


def test_discontinuity_closed_forms():
    const = np.full((9, 11), -320, np.int16)
    dd = wn.discontinuity(const, 4, 0.001)
    # mean^2 and the mean of squares round alike only approximately in float: |var| <= 2 ulp of 320^2
    assert np.abs(dd - 1).max() <= 0.001 * 2 * np.spacing(f32(320.0 ** 2)) + np.finfo(f32).eps
    # a two-level step: a window with k of its N cells at B and the rest at A has variance p (1 - p) (B - A)^2
    A, B, r = 160, 480, 2
    step = np.full((20, 30), A, np.int16)
    step[:, 15:] = B
    dd = wn.discontinuity(step, r, 0.001)
    for x in (5, 13, 14, 15, 16, 25):
        k = np.clip(x + r - 14, 0, 2 * r + 1)   # columns of the window at B
        pfrac = k / (2 * r + 1)
        want = max(0.0, 1 - 0.001 * pfrac * (1 - pfrac) * (B - A) ** 2)
        assert abs(dd[10, x] - want) < 1e-4, x
    assert wn.discontinuity(np.array([[5]], np.int16), 3, 0.001)[0, 0] == 1    # a crop of one pixel reflects onto itself
    assert np.array_equal(wn.reflect101(np.arange(-4, 8), 4), [2, 3, 2, 1, 0, 1, 2, 3, 2, 1, 0, 1])


def test_confidence_on_hand_built_maps():
    h, w = 8, 40
    p = wn.WlsParams(depth_discontinuity_radius=1, roi_left=10, roi_right=2, roi_top=1, roi_bottom=1)
    x0, y0, rw, rh = wn.roi(p, w, h)
    assert (x0, y0, rw, rh) == (10, 1, 28, 6)
    xr0 = w - (x0 + rw)
    assert xr0 == 2
    dl = np.full((h, w), 5 * 16, np.int16)
    dr = np.full((h, w), -5 * 16, np.int16)
    conf = wn.confidence(dl, dr, p)
    # consistent, flat: dd = 1 on both sides, wherever x - 5 lies in the right ROI (columns 2..29)
    assert (conf[:, :25] == 1).all() and (conf[:, 25:] == 0).all()
    dr2 = dr.copy()
    dr2[3, 20 - 5] = -5 * 16 - 24                  # |dl + dr| = 24 is not < 24
    dr2[4, 20 - 5] = -5 * 16 - 23
    conf = wn.confidence(dl, dr2, p)
    assert conf[3 - y0, 20 - x0] == 0
    assert 0 < conf[4 - y0, 20 - x0] < 1           # kept, lowered by the right map's local variance
    dl3 = dl.copy()
    dl3[2, 12] = 11 * 16 + 7                       # xr = 12 - 11 = 1 < xr0: outside the right ROI
    dl3[2, 13] = -30 * 16                          # xr = 13 + 30 = 43 >= w
    dl3[5, 20] = -2 * 16                           # the left matcher's invalid value with min_disparity -1: inconsistent
    conf = wn.confidence(dl3, dr, p)
    assert conf[2 - y0, 12 - x0] == 0 and conf[2 - y0, 13 - x0] == 0 and conf[5 - y0, 20 - x0] == 0
    # its neighbours pay through dd_left: eight cells at 80 and one at -32 have variance 1238 -> dd = max(0, 1 - 1.238)
    assert conf[5 - y0, 21 - x0] == 0 and conf[4 - y0, 19 - x0] == 0 and conf[5 - y0, 22 - x0] == 1


def test_confidence_right_roi_bound():
    p = wn.WlsParams(depth_discontinuity_radius=0, roi_left=10, roi_right=2, roi_top=0, roi_bottom=0)
    dl = np.full((2, 40), 5 * 16, np.int16)
    dr = np.full((2, 40), -5 * 16, np.int16)
    conf = wn.confidence(dl, dr, p)
    # right ROI = columns 2..29: left pixels x with x - 5 in 2..29, i.e. x <= 34, are kept
    assert (conf[:, :25] == 1).all() and (conf[:, 25:] == 0).all()


def test_parameters_of_the_references_matcher():
    left = sn.Params()
    r = wn.right_matcher_params(left)
    assert (r.min_disparity, r.num_disparities, r.block_size, r.p1, r.p2, r.disp12_max_diff, r.pre_filter_cap,
            r.uniqueness_ratio, r.speckle_window_size, r.speckle_range, r.mode) == (-96, 96, 7, 24, 96, 1000000, 60, 0, 0, 0, 0)
    p = wn.default_params(left)
    assert (p.lambda_, p.sigma_color, p.use_confidence, p.lrc_thresh, p.depth_discontinuity_radius) == (8000.0, 1.5, 1, 24, 4)
    assert f32(p.roll_off) == f32(0.001)
    assert (p.roi_left, p.roi_right, p.roi_top, p.roi_bottom) == (100, 3, 3, 3)
    assert wn.roi(p, 1241, 376) == (100, 3, 1138, 370)
    q = wn.default_params(sn.Params(min_disparity=-8, num_disparities=32, block_size=3))
    assert (q.roi_left, q.roi_right, q.roi_top, q.depth_discontinuity_radius) == (25, 9, 1, 2)
    assert wn.lambda_ref(8000.0) == f32(1.5 * 8000.0 * 16 / 63)
    t1, t3 = wn.lut(1.5, 1), wn.lut(1.5, 3)
    assert t1.shape == (256,) and t3.shape == (3 * 255 * 255 + 1,) and t1[0] == -1 and t3[0] == -1
    assert np.array_equal(t3[np.arange(256) ** 2], t1)   # sqrt of a perfect square is exact
    assert np.abs(t1 + np.exp(-np.arange(256) / 1.5)).max() < 1e-7
