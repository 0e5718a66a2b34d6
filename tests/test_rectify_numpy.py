"""The numpy restatement of the rectification chain (tests/rectify_numpy.py) against definitions, not against itself: Rodrigues
against scipy, the rectified cameras against the raw camera model on 3-D points (the known-answer test), Q, the identity case
against svo_stereo_rectify_q, the inverse model, the fixed-point conversion at every boundary, the weights against OpenCV's table
construction, remap against a literal loop, and the proof that every fixture reaches the branch it is named for.  CPU only."""
import ctypes as C

import numpy as np
import pytest
from scipy.spatial.transform import Rotation as Rot

import rectify_fixtures as rf
import rectify_numpy as rn
from ros_stereo_slam_amd import capi

RIGS = sorted(rf.RIGS)


def test_rodrigues_against_scipy():
    rng = np.random.default_rng(1)
    vs = [rng.normal(size=3) * s for s in (1e-9, 1e-3, 0.02, 0.5, 2.0, 3.0) for _ in range(5)]
    for v in vs:
        R = rn.rodrigues(v)
        assert np.abs(R - Rot.from_rotvec(v).as_matrix()).max() < 1e-15 * 8
        if np.linalg.norm(v) > 1e-4:   # below s = 1e-5 upstream returns zero (N3)
            assert np.abs(rn.rodrigues(rn.rodrigues(R)) - R).max() < 1e-11   # the vector itself is unique only below pi
    assert np.array_equal(rn.rodrigues(np.zeros(3)), np.eye(3)) and np.array_equal(rn.rodrigues(np.eye(3)), np.zeros(3))
    for axis in ([1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [1, -2, 3]):   # half turns: the diagonal form
        a = np.array(axis, float) / np.linalg.norm(axis) * np.pi
        v = rn.rodrigues(Rot.from_rotvec(a).as_matrix())
        assert min(np.abs(v - a).max(), np.abs(v + a).max()) < 1e-7


@pytest.mark.parametrize("name", RIGS)
def test_rotations_and_baseline(name):
    _, _, _, _, _, R, T = rf.RIGS[name]
    R1, R2, P1, P2, Q = rf.rectification(name)
    for Ri in (R1, R2):
        assert np.abs(Ri @ Ri.T - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(Ri) - 1) < 1e-14
    t = R2 @ T
    idx = 1 if name == "vertical" else 0
    off = np.delete(t, idx)
    assert np.abs(off).max() <= 1e-12 * np.linalg.norm(T) and abs(abs(t[idx]) - np.linalg.norm(T)) <= 1e-12
    assert abs(P2[idx, 3] - t[idx] * P1[0, 0]) <= 1e-13 * abs(P2[idx, 3]) and P2[idx ^ 1, 3] == 0 and P1[0, 0] == P1[1, 1] == P2[0, 0]
    if name == "identity":
        assert np.array_equal(R1, np.eye(3)) and np.array_equal(R2, np.eye(3))


def raw_pixel(X, K, D, R=None, T=None):
    """a 3-D point of the first camera's frame through a raw camera, plain numpy"""
    Xc = X if R is None else X @ np.asarray(R).T + T
    return rn.distort(Xc[:, 0] / Xc[:, 2], Xc[:, 1] / Xc[:, 2], K, D)


@pytest.mark.parametrize("name", RIGS)
def test_forward_consistency(name):
    """The known-answer test: a 3-D point seen by the raw camera lands where the rectified camera's pixel says the map reads."""
    K1, D1, K2, D2, size, R, T = rf.RIGS[name]
    R1, R2, P1, P2, Q = rf.rectification(name)
    idx = 1 if name == "vertical" else 0
    gx, gy, gz = np.meshgrid(np.linspace(-1.2, 1.2, 9), np.linspace(-0.8, 0.8, 7), [1.5, 3.0, 10.0, 40.0])
    X = np.stack([gx.ravel() * gz.ravel() / 3, gy.ravel() * gz.ravel() / 3, gz.ravel()], 1)
    # the rectified pixel of the point in both cameras: P_i R_i x_i
    Xr1, Xr2 = X @ R1.T, (X @ R.T + T) @ R2.T
    pr = []
    for Xr, P in ((Xr1, P1), (Xr2, P2)):
        h = Xr @ P[:, :3].T   # each camera's own rectified frame: P's fourth column places camera 2 in camera 1's
        pr.append(h[:, :2] / h[:, 2:])
    worst = 0.0
    for (px, K, D, Ri, P, raw) in ((pr[0], K1, D1, R1, P1, raw_pixel(X, K1, D1)), (pr[1], K2, D2, R2, P2, raw_pixel(X, K2, D2, R, T))):
        # R3's unrounded (u, v) at the (non-integer) rectified pixel
        iR = rn.inv3(rn.mat3(P[:, :3], Ri))
        Xn = px[:, 0] * iR[0, 0] + (px[:, 1] * iR[0, 1] + iR[0, 2])
        Yn = px[:, 0] * iR[1, 0] + (px[:, 1] * iR[1, 1] + iR[1, 2])
        Wn = px[:, 0] * iR[2, 0] + (px[:, 1] * iR[2, 1] + iR[2, 2])
        u, v = rn.distort(Xn / Wn, Yn / Wn, K, D)
        worst = max(worst, np.abs(u - raw[0]).max(), np.abs(v - raw[1]).max())
    print(f"{name}: raw pixel against the map's source coordinate, worst {worst:.3e} px")
    assert worst <= 1e-8
    # the rows (columns for a vertical rig) agree, and the disparity is -P2[idx][3] / Z
    assert np.abs(pr[0][:, idx ^ 1] - pr[1][:, idx ^ 1]).max() <= 1e-8
    Z = Xr1[:, 2]
    assert np.abs((pr[0][:, idx] - pr[1][:, idx]) - (-P2[idx, 3] / Z)).max() <= 1e-8
    # Q maps (u, v, d) back to R1 X
    d = pr[0][:, idx] - pr[1][:, idx]
    hom = np.stack([pr[0][:, 0], pr[0][:, 1], d, np.ones_like(d)], 1) @ Q.T
    assert np.abs(hom[:, :3] / hom[:, 3:] - Xr1).max() <= 1e-8 * 40


def test_identity_q_equals_stereo_rectify_q():
    K = rf.RIGS["identity"][0]
    Q = np.zeros(16)
    capi._check(capi.load().svo_stereo_rectify_q(C.c_double(K[0, 0]), C.c_double(K[1, 1]), C.c_double(K[0, 2]), C.c_double(K[1, 2]),
                                                 C.c_double(-0.54), 1241, 376, capi._ptr(Q)))
    assert np.abs(rf.rectification("identity")[4].ravel() - Q).max() <= 1e-9


def test_flags_and_new_size():
    K1, D1, K2, D2, size, R, T = rf.RIGS["euroc"]
    a = rn.stereo_rectify(K1, D1, K2, D2, size, R, T, flags=0)
    z = rf.rectification("euroc")
    assert a[2][1, 2] == a[3][1, 2] and a[2][0, 2] != a[3][0, 2] and a[4][3, 3] != 0      # only y is shared; Q carries the offset
    assert z[2][0, 2] == z[3][0, 2] and z[4][3, 3] == 0
    b = rn.stereo_rectify(K1, D1, K2, D2, size, R, T, new_size=(376, 240))
    assert all(np.array_equal(p, q) for p, q in zip(b, z))                                  # N7
    with pytest.raises(ValueError):
        rn.stereo_rectify(K1, D1, K2, D2, size, R, T, alpha=0.0)
    with pytest.raises(ValueError):
        rn.coeffs(np.zeros(12))


@pytest.mark.parametrize("name", RIGS)
def test_undistort_inverts_the_model(name):
    """the residual of undistort -> distort falls with every iteration; its value after five is printed, not asserted (DESIGN.md
    section 10p quotes it)"""
    K, D, _, _, size, _, _ = rf.RIGS[name]
    j, i = np.meshgrid(np.linspace(0, size[0] - 1, 23), np.linspace(0, size[1] - 1, 17))
    pts = np.stack([j.ravel(), i.ravel()], 1).astype(np.float32)
    res = []
    for it in range(1, 6):
        n = rn.undistort_points(pts, K, D, iters=it)
        u, v = rn.distort(n[:, 0], n[:, 1], K, D)
        res.append(max(np.abs(u - pts[:, 0]).max(), np.abs(v - pts[:, 1]).max()))
    print(f"{name}: undistort -> distort residual per iteration (px): " + " ".join(f"{r:.3e}" for r in res))
    if rn.coeffs(D).any():
        assert all(b < a for a, b in zip(res, res[1:]))
    else:
        assert max(res) < 1e-10


def test_fixed_point_boundaries():
    # u * 32 exactly on .5: both parities of the even rule
    assert rn.fix5(np.array([1 / 64, 3 / 64, 5 / 64, -1 / 64, -3 / 64])).tolist() == [0, 2, 2, 0, -2]
    # negative coordinates: the shift and the mask agree with floor semantics
    for v in (-1 / 32, -0.5, -1.0, -1 - 1 / 32, -33 / 32, -7.25):
        xy, fr = rn.fixed_maps(np.array([[v]]), np.array([[v]]))
        assert xy[0, 0, 0] == np.floor(v) and (fr[0, 0] & 31) == round((v - np.floor(v)) * 32) and xy[0, 0, 0] + (fr[0, 0] & 31) / 32 == v
    # +-32767 and beyond, NaN, infinities
    big = np.array([[32767.0, 32767.99, 32768.0, 1e6, -32768.0, -32768.04, -1e6, 67108863.9, 67108864.0, -67108864.0, -67108865.0,
                     np.nan, np.inf, -np.inf]])
    xy, fr = rn.fixed_maps(big, np.zeros_like(big))
    assert xy[0, :, 0].tolist() == [32767, 32767, 32767, 32767, -32768, -32768, -32768, 32767, -32768, -32768, -32768, -32768,
                                    -32768, -32768]
    assert (fr[0] & 31).tolist() == [0, 0, 0, 0, 0, 31, 0, 29, 0, 0, 0, 0, 0, 0]   # 67108863.9 x 32 rounds to 2^31 - 3
    assert rn.fix5(np.array([67108863.99])).tolist() == [rn.INT_MIN]                 # rounds to 2^31: overflows
    # the float conversion of the boundary fixture is self-consistent with the word form
    xy, fr = rn.float_maps(rf.BOUNDARY[None], rf.BOUNDARY[None, ::-1])
    assert xy.dtype == np.int16 and fr.dtype == np.uint16 and fr.max() < 1024


def test_weights_equal_the_table_construction():
    tab, fired = rn.cv_weight_table()
    ours = np.stack(rn.weights(np.arange(1024)), 1)
    assert np.array_equal(tab, ours) and (ours.sum(1) == 1 << 15).all()
    # the correction fires nowhere but at fraction (0, 0), where saturate_cast<short> cuts 2^15 and the correction restores it;
    # as 32767 or as 2^15 the weight gives the same pixel for every byte
    assert fired == [0]
    p = np.arange(256)
    assert np.array_equal((32768 * p + (1 << 14)) >> 15, p) and np.array_equal((32767 * p + (1 << 14)) >> 15, p)


@pytest.mark.parametrize("c", [1, 3])
def test_remap_against_the_literal_loop(c):
    for name in rf.HAND_MAPS:
        for (w, h, sw, sh) in ((32, 32, 9, 7), (13, 5, 1, 1), (7, 3, 2, 2)):
            xy, fr = rf.hand_maps(name, w, h, sw, sh, seed=3)
            src = rf.source(sw, sh, c, 5)
            for value in (0, 7, 255):
                assert np.array_equal(rn.remap(src, xy, fr, value), rn.remap_loop(src, xy, fr, value)), (name, w, h, sw, sh, value)
    xy, fr = rf.hand_maps("identity", 9, 7, 9, 7)
    src = rf.source(9, 7, c, 1)
    assert np.array_equal(rn.remap(src, xy, fr, 99), src)   # the taps at x + 1 / y + 1 carry weight 0


def test_fixtures_reach_their_branches():
    sw, sh = 9, 7
    fast = lambda xy: ((xy[..., 0] >= 0) & (xy[..., 0] < sw - 1) & (xy[..., 1] >= 0) & (xy[..., 1] < sh - 1))
    quads = lambda a: a.reshape(a.shape[0], -1, 4)
    # a thread whose four pixels straddle the fast and the bordered path
    xy, _ = rf.hand_maps("one_tap_inside", 32, 32, sw, sh)
    f = quads(fast(xy))
    assert (f[..., :3].all(-1) & ~f[..., 3]).any()
    # windows with 2 taps outside on each of the four sides and 3 at the corners.  Exactly ONE tap outside cannot happen: the
    # window and the source are axis-aligned rectangles, so taps leave a column or a row at a time (asserted over every position)
    xy, _ = rf.hand_maps("half_outside", 32, 32, sw, sh)
    x, y, out = xy[..., 0], xy[..., 1], rn.taps_outside(xy, (sw, sh))
    for side in (x == -1, x == sw - 1, y == -1, y == sh - 1):
        assert (side & (out == 2)).any()
    assert (out == 3).any()
    xy, _ = rf.hand_maps("one_tap_inside", 32, 32, sw, sh)
    assert {0, 2, 3} <= set(np.unique(rn.taps_outside(xy, (sw, sh))).tolist())
    jj, ii = np.meshgrid(np.arange(-3, sw + 3), np.arange(-3, sh + 3))
    assert set(np.unique(rn.taps_outside(np.stack([jj, ii], -1), (sw, sh))).tolist()) == {0, 2, 3, 4}
    # a map that is fully outside
    xy, _ = rf.hand_maps("outside", 32, 32, sw, sh)
    assert (rn.taps_outside(xy, (sw, sh)) == 4).all()
    # every fraction pair
    _, fr = rf.hand_maps("fractions", 32, 32, sw, sh)
    assert len(np.unique(fr)) == 1024
    # the rig maps hold fast quads, bordered quads and quads that straddle them
    (xy, _), _ = rf.rig_maps("euroc")
    f = quads(fast(xy).astype(bool) & (rn.taps_outside(xy, (752, 480)) == 0))
    assert f.all(-1).any() and (~f).all(-1).any() and (f.any(-1) & ~f.all(-1)).any()
