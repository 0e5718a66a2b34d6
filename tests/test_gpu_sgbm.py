"""The dense stereo matcher and the reprojection (svo_sgbm_compute / svo_stereo_reproject, StereoProcess of
src/StereoCV.cpp:21-59,227-250) bit for bit against the numpy restatement tests/sgbm_numpy.py."""
import numpy as np
import pytest

import sgbm_numpy as sn
from ros_stereo_slam_amd import capi, synth

pytestmark = pytest.mark.gpu


def _pair(w, h, c=1, shift=7, seed=1, noise=6):
    a, b = synth.textured_pair(w, h, c, shift=(shift, 0), seed=seed, colour=c == 3)
    rng = np.random.default_rng(seed)
    # the left image sees the texture shifted right; a little noise so costs tie rarely but not never
    left = np.clip(b.astype(np.int32) + rng.integers(-noise, noise + 1, b.shape), 0, 255).astype(np.uint8)
    right = np.clip(a.astype(np.int32) + rng.integers(-noise, noise + 1, a.shape), 0, 255).astype(np.uint8)
    return left, right


def _params(**kw):
    p = sn.Params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _check(ctx, left, right, **kw):
    want = sn.sgbm(left, right, _params(**kw))
    got = ctx.sgbm(left, right, **kw)
    assert got.dtype == np.int16 and got.shape == want.shape
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        y, x = bad[0]
        raise AssertionError(f"{len(bad)} pixels differ, first ({y}, {x}): got {got[y, x]} want {want[y, x]}")
    return got


@pytest.fixture(scope="module")
def kitti_pair():
    scene = synth.Scene()
    left, right, _ = scene.stereo(np.eye(3), np.zeros(3), channels=3)
    return left, right


@pytest.mark.parametrize("grey", [True, False], ids=["grey", "bgr"])
def test_reference_parameters_full_size(ctx, kitti_pair, grey):
    left, right = kitti_pair
    if grey:
        left, right = sn.cv_gray(left), sn.cv_gray(right)
    got = _check(ctx, left, right)
    assert (got > 0).mean() > 0.3   # the matcher found something


@pytest.mark.parametrize("D", [16, 64, 96, 256])
def test_num_disparities(ctx, D):
    left, right = _pair(D + 90, 24, shift=min(9, D - 4))
    _check(ctx, left, right, num_disparities=D, speckle_window_size=0)


@pytest.mark.parametrize("minD", [0, 1, -8])
@pytest.mark.parametrize("block", [1, 3, 7, 11])
def test_min_disparity_and_block(ctx, minD, block):
    left, right = _pair(150, 30, shift=6, seed=block + 3)
    _check(ctx, left, right, min_disparity=minD, num_disparities=32, block_size=block, speckle_window_size=0)


@pytest.mark.parametrize("ratio", [0, 10])
@pytest.mark.parametrize("speckle", [0, 40])
@pytest.mark.parametrize("maxdiff", [-1, 0, 2])
def test_uniqueness_speckle_lr(ctx, ratio, speckle, maxdiff):
    left, right = _pair(160, 32, shift=5, seed=11, noise=20)
    _check(ctx, left, right, num_disparities=48, uniqueness_ratio=ratio, speckle_window_size=speckle, speckle_range=2,
           disp12_max_diff=maxdiff)


@pytest.mark.parametrize("w,h", [(98, 20), (99, 9), (131, 17), (201, 1), (203, 2), (90, 5)])
def test_narrow_odd_and_flat_shapes(ctx, w, h):
    left, right = _pair(w, h, shift=3, seed=w)
    minD = -8 if w == 90 else 1   # 90 > 96 - 8 passes the argument check, the band is empty: all invalid
    _check(ctx, left, right, min_disparity=minD, speckle_window_size=5 if h > 2 else 0)


def test_batch_of_16(ctx):
    pairs = [_pair(180, 28, c=3, shift=3 + k % 5, seed=40 + k) for k in range(16)]
    L = np.stack([p[0] for p in pairs])
    R = np.stack([p[1] for p in pairs])
    kw = dict(num_disparities=32, speckle_window_size=30)
    batch = ctx.sgbm(L, R, **kw)
    assert batch.shape == (16, 28, 180)
    for k in range(16):
        one = ctx.sgbm(L[k], R[k], **kw)
        assert np.array_equal(batch[k], one), k
        assert np.array_equal(one, sn.sgbm(L[k], R[k], _params(**kw))), k


def test_device_memory_matches_host(ctx):
    import torch

    left, right = _pair(300, 40, c=3, shift=8, seed=5)
    host = ctx.sgbm(left, right, num_disparities=64, speckle_window_size=50)
    dl, dr = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
    dev = ctx.sgbm(dl, dr, num_disparities=64, speckle_window_size=50)
    assert dev.is_cuda and dev.dtype == torch.int16
    assert np.array_equal(dev.cpu().numpy(), host)


@pytest.mark.parametrize("which", ["reference", "metric"])
def test_reprojection_exact(ctx, kitti_pair, which):
    left, right = kitti_pair
    disp = ctx.sgbm(left, right)
    fx, fy, cx, cy = synth.KITTI_K
    B = 0.5707
    if which == "reference":
        Q, scale = capi.stereo_rectify_q(fx, fy, cx, cy, B, 1241, 376), 1.0
    else:
        Q, scale = capi.stereo_rectify_q(fx, fy, cx, cy, -B, 1241, 376), 1.0 / 16
    assert np.array_equal(Q, sn.stereo_rectify_q(fx, fy, cx, cy, B if which == "reference" else -B, 1241, 376))
    for zmin, zmax in ((0.01, 5.0), (0.01, 80.0), (-1e30, 1e30)):
        xg, cg = ctx.stereo_reproject(disp, left, Q, disp_scale=scale, z_min=zmin, z_max=zmax)
        xw, cw = sn.reproject(disp, left, Q, disp_scale=scale, z_min=zmin, z_max=zmax)
        assert len(xg) == len(xw)
        assert np.array_equal(xg, xw, equal_nan=True) and np.array_equal(cg, cw)
    if which == "reference":
        # t = +baseline: every valid disparity reprojects behind the camera, the (0.01, 5] window keeps nothing
        assert len(ctx.stereo_reproject(disp, left, Q)[0]) == 0
    else:
        assert len(ctx.stereo_reproject(disp, left, Q, disp_scale=scale, z_max=80.0)[0]) > 10000


def test_reprojection_grey_and_no_flip(ctx):
    rng = np.random.default_rng(3)
    disp = rng.integers(-20, 1500, (50, 70)).astype(np.int16)
    img = rng.integers(0, 256, (50, 70), dtype=np.uint8)
    Q = capi.stereo_rectify_q(500.0, 510.0, 33.3, 24.1, -0.3, 70, 50)
    xg, cg = ctx.stereo_reproject(disp, img, Q, disp_scale=1 / 16, z_min=0.5, z_max=40.0, flip_y=False)
    xw, cw = sn.reproject(disp, img, Q, disp_scale=1 / 16, z_min=0.5, z_max=40.0, flip_y=False)
    assert len(xg) == len(xw) > 0
    assert np.array_equal(xg, xw) and np.array_equal(cg, cw)


@pytest.mark.parametrize("bad", [dict(num_disparities=0), dict(num_disparities=40), dict(num_disparities=272),
                                 dict(block_size=4), dict(block_size=13), dict(block_size=-1), dict(p1=96, p2=96),
                                 dict(p1=100, p2=50), dict(mode=1), dict(min_disparity=30, num_disparities=96)])
def test_bad_arguments_refused(ctx, bad):
    left, right = _pair(126, 8)
    with pytest.raises(capi.SvoError) as e:
        ctx.sgbm(left, right, **bad)
    assert e.value.code == capi.SVO_ERR_ARG
