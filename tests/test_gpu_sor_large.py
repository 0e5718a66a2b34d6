"""svo_sor_filter_large on the GPU: the same bits as svo_sor_filter and the oracle where they overlap (n <= 9216), the
same bits as the numpy restatement (tests/sor_numpy.py) beyond, degenerate clouds that must finish, device memory,
and the argument limits."""
import ctypes as C

import numpy as np
import pytest

import sor_numpy as sn
from ros_stereo_slam_amd import capi, synth
from test_oracle_sor import cloud

pytestmark = pytest.mark.gpu


def depth_cloud(n, seed=0, outliers=0.01):
    """n points sampled like a depth map over noisy planes and boxes (ground, a wall, two boxes), in metres with the
    camera's z forward, plus a fraction of outliers scattered through the scene's bounding box."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(n)))
    u, v = np.meshgrid(np.linspace(-1, 1, side), np.linspace(0, 1, side))
    u, v = u.ravel()[:n], v.ravel()[:n]
    kind = rng.integers(0, 4, n)
    pts = np.empty((n, 3))
    g = kind == 0                                          # ground: y = -1.6, depth 2..40 m
    pts[g] = np.stack([u[g] * 15, np.full(g.sum(), -1.6), 2 + 38 * v[g]], 1)
    w = kind == 1                                          # wall: z = 30
    pts[w] = np.stack([u[w] * 20, -1.6 + 8 * v[w], np.full(w.sum(), 30.0)], 1)
    b = kind == 2                                          # box front face: z = 8
    pts[b] = np.stack([-3 + 2 * u[b], -1.6 + 2 * v[b], np.full(b.sum(), 8.0)], 1)
    s = kind == 3                                          # box side face: x = 4
    pts[s] = np.stack([np.full(s.sum(), 4.0), -1.6 + 3 * v[s], 10 + 5 * u[s]], 1)
    pts += rng.normal(0, 0.01, pts.shape)
    k = int(n * outliers)
    if k:
        lo, hi = pts.min(0), pts.max(0)
        pts[rng.choice(n, k, replace=False)] = lo + (hi - lo) * rng.random((k, 3))
    col = rng.integers(0, 256, (n, 3)).astype(np.float32)
    return pts.astype(np.float32), col


def same(a, b):
    assert len(a[2]) == len(b[2])
    assert np.array_equal(a[2], b[2])                     # float32 mean distances, bit for bit
    assert np.array_equal(a[0], b[0])
    assert (a[1] is None and b[1] is None) or np.array_equal(a[1], b[1])


@pytest.mark.parametrize("n", [4428, 1500, 1000, 300, 150, 64, 2, 1, 9216])
@pytest.mark.parametrize("k", [200, 20])
def test_matches_brute_force_and_oracle(ctx, orc, n, k):
    xyz, col = cloud(n, seed=n + 1, outliers=n // 40)
    large = ctx.sor_filter_large(xyz, col, mean_k=k, stddev_mul=0.01, z_limit=500.0)
    same(large, ctx.sor_filter(xyz, col, mean_k=k, stddev_mul=0.01, z_limit=500.0))
    same(large, orc.sor_filter(xyz, col, mean_k=k, stddev_mul=0.01, z_limit=500.0))


@pytest.mark.parametrize("n,ks", [(9217, (1, 20, 200, 256)), (50000, (1, 20, 256)), (200000, (20, 200)),
                                  (466616, (20, 256))])
def test_large_clouds_match_restatement(ctx, n, ks):
    xyz, col = depth_cloud(n, seed=n)
    for k in ks:
        same(ctx.sor_filter_large(xyz, col, mean_k=k), sn.sor_filter(xyz, col, mean_k=k))


def _dense_scene_cloud(ctx):
    left, right, _ = synth.Scene().stereo(np.eye(3), np.zeros(3), channels=3)
    disp = ctx.sgbm(left, right)
    fx, fy, cx, cy = synth.KITTI_K
    Q = capi.stereo_rectify_q(fx, fy, cx, cy, -0.5707, 1241, 376)
    return disp, left, Q


def test_dense_scene_cloud(ctx):
    disp, left, Q = _dense_scene_cloud(ctx)
    xyz, bgr = ctx.stereo_reproject(disp, left, Q, disp_scale=1 / 16, z_max=80.0)
    assert len(xyz) > 10000
    same(ctx.sor_filter_large(xyz, bgr), sn.sor_filter(xyz, bgr))
    same(ctx.sor_filter_large(xyz, bgr, mean_k=200, stddev_mul=0.01), sn.sor_filter(xyz, bgr, 200, 0.01))


def test_device_memory_equals_host(ctx):
    """Fed from svo_stereo_reproject's device outputs: the same bits as the host path."""
    import torch

    disp, left, Q = _dense_scene_cloud(ctx)
    h, w = disp.shape
    d_disp = torch.from_numpy(disp).cuda()
    d_img = torch.from_numpy(np.ascontiguousarray(left)).cuda()
    d_xyz = torch.empty((h * w, 3), dtype=torch.float32, device="cuda")
    d_bgr = torch.empty_like(d_xyz)
    q = np.ascontiguousarray(Q, np.float64).reshape(16)
    n = C.c_int()
    torch.cuda.synchronize()
    capi._check(ctx.lib.svo_stereo_reproject(ctx._h, capi._ptr(d_disp), capi._ptr(d_img), w, h, 3, capi._ptr(q),
                                             C.c_float(1 / 16), C.c_float(0.01), C.c_float(80.0), 1, capi._ptr(d_xyz),
                                             capi._ptr(d_bgr), C.byref(n), capi.MEM_DEVICE))
    capi._check(ctx.lib.svo_ctx_sync(ctx._h))
    d_xyz, d_bgr = d_xyz[:n.value], d_bgr[:n.value]
    xd, cd, md = ctx.sor_filter_large(d_xyz, d_bgr)
    assert xd.is_cuda and cd.is_cuda and md.is_cuda
    host = ctx.sor_filter_large(d_xyz.cpu().numpy(), d_bgr.cpu().numpy())
    same((xd.cpu().numpy(), cd.cpu().numpy(), md.cpu().numpy()), host)
    xd, cd, md = ctx.sor_filter_large(d_xyz[:0], None)
    assert len(xd) == 0 and cd is None and len(md) == 0


def _line(n, rng):
    t = rng.random(n).astype(np.float32)
    return np.stack([t * 3, t * 2 - 1, -5 - t], 1).astype(np.float32)


def _degenerate():
    rng = np.random.default_rng(9)
    base, _ = depth_cloud(20000, seed=4, outliers=0.0)
    far = base.copy()
    far[123] = (1e6, -1e6, 1e6)
    spread = base.copy()
    spread[rng.choice(len(base), 30, replace=False)] *= 1e4
    plane = rng.random((20000, 3)).astype(np.float32)
    plane[:, 2] = -2.0
    lattice = np.stack(np.meshgrid(np.arange(20), np.arange(20), np.arange(20), indexing="ij"), -1).reshape(-1, 3)
    return {"identical": np.full((3000, 3), 1.5, np.float32),
            "identical_pairs": np.repeat(rng.normal(0, 1, (1500, 3)).astype(np.float32), 2, axis=0),
            "collinear": _line(20000, rng), "coplanar": plane, "one_far_point": far, "box_1e4_wider": spread,
            "lattice": lattice.astype(np.float32) * 0.5}


@pytest.mark.parametrize("name", ["identical", "identical_pairs", "collinear", "coplanar", "one_far_point",
                                  "box_1e4_wider", "lattice"])
@pytest.mark.parametrize("k", [20, 256])
def test_degenerate_clouds_finish_exact(ctx, name, k):
    xyz = _degenerate()[name]
    same(ctx.sor_filter_large(xyz, mean_k=k), sn.sor_filter(xyz, mean_k=k))


@pytest.mark.parametrize("m", [0, 1, 2, 3, 20, 21, 256, 257])
def test_few_points(ctx, m):
    xyz, col = cloud(max(m, 1), seed=m)
    xyz, col = xyz[:m], col[:m]
    for k in (1, 20, 256):
        same(ctx.sor_filter_large(xyz, col, mean_k=k), sn.sor_filter(xyz, col, mean_k=k))


def test_prefilter_all_dropped_and_non_finite(ctx):
    x, c, d = ctx.sor_filter_large(np.array([[0, 0, -600.0]] * 7, np.float32), np.ones((7, 3), np.float32),
                                   z_limit=500.0)
    assert len(x) == len(c) == len(d) == 0
    xyz, col = depth_cloud(30000, seed=2)
    xyz[1000] = (np.nan, 0, 1)
    xyz[2000] = (0, np.inf, 1)
    xyz[3000] = (0, 0, -np.inf)
    xyz[4000, 2] = -900.0
    out = ctx.sor_filter_large(xyz, col, z_limit=500.0)
    assert len(out[2]) == len(xyz) - 4
    same(out, sn.sor_filter(xyz, col, z_limit=500.0))


def test_limits(ctx):
    big = np.zeros(((1 << 22) + 1, 3), np.float32)
    with pytest.raises(capi.SvoError) as e:
        ctx.sor_filter_large(big)
    assert e.value.code == capi.SVO_ERR_CAPACITY
    xyz, _ = cloud(100, seed=1)
    for k in (0, 257):
        with pytest.raises(capi.SvoError) as e:
            ctx.sor_filter_large(xyz, mean_k=k)
        assert e.value.code == capi.SVO_ERR_ARG
    same(ctx.sor_filter_large(xyz, mean_k=256), sn.sor_filter(xyz, mean_k=256))
