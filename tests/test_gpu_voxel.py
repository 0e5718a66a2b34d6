"""svo_voxel_downsample on the GPU, bit for bit against the numpy restatement (tests/voxel_numpy.py): every fixture of
tests/voxel_fixtures.py and the sizes around every tile seam, with and without colours and the trace, in host and device memory behind
sentinel guard bands; repeatability, two contexts, buffer reuse, the refusals, the neighbours on the same context
(svo_sor_filter_large, svo_cloud) keeping their bits, PoseGraphOptimize(voxel_down_sample=True) and the C++ adaptor."""
import ctypes as C
import itertools
import pathlib
import subprocess

import numpy as np
import pytest

import icp_fixtures as icp_fx
import voxel_fixtures as vf
import voxel_numpy as vn
from ros_stereo_slam_amd import capi, registration

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parents[1]
GUARD = 5                       # rows in front of and behind every output
F_SENT, I_SENT = np.float32(-777.25), np.int32(-12345)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def run_guarded(ctx, xyz, col, leaf, trace, device):
    """the raw entry point with every output placed between two sentinel bands and filled with the sentinel; checks the bands and the
    rows past n_out, -> (rc, xyz_out, color_out, point_voxel, voxel_count)"""
    import torch

    n = len(xyz)
    rows = n + 2 * GUARD
    host = dict(xo=np.full((rows, 3), F_SENT), co=np.full((rows, 3), F_SENT) if col is not None else None,
                pv=np.full(rows, I_SENT) if trace else None, vc=np.full(rows, I_SENT) if trace else None)
    if device:
        dev = torch.device("cuda", 0)
        bufs = {k: (None if v is None else torch.from_numpy(v).to(dev)) for k, v in host.items()}
        xin = torch.from_numpy(np.ascontiguousarray(xyz)).to(dev) if n else None
        cin = torch.from_numpy(np.ascontiguousarray(col)).to(dev) if col is not None and n else None
        torch.cuda.synchronize()
        base = lambda t: None if t is None else t.data_ptr()
        step = lambda t: t.element_size() * (t.shape[1] if t.dim() == 2 else 1)
    else:
        bufs = host
        xin, cin = (np.ascontiguousarray(xyz) if n else None), (np.ascontiguousarray(col) if col is not None and n else None)
        base = lambda a: None if a is None else a.ctypes.data
        step = lambda a: a.strides[0]
    ptr = lambda a: C.c_void_p(0) if a is None else C.c_void_p(base(a) + GUARD * step(a))
    inp = lambda a: C.c_void_p(0) if a is None else C.c_void_p(base(a))
    n_out = C.c_int(-9)
    rc = ctx.lib.svo_voxel_downsample(ctx._h, inp(xin), inp(cin), n, C.c_double(leaf), ptr(bufs["xo"]),
                                      ptr(bufs["co"]), C.byref(n_out),
                                      ptr(bufs["pv"]), ptr(bufs["vc"]), capi.MEM_DEVICE if device else capi.MEM_HOST)
    got = {k: (None if v is None else (v.cpu().numpy() if device else v)) for k, v in bufs.items()}
    if rc != capi.SVO_OK:
        assert n_out.value == -9
        for k, v in got.items():
            assert v is None or (v == (F_SENT if v.dtype == np.float32 else I_SENT)).all(), f"{k} written by a refused call"
        return rc, None, None, None, None
    k_out = n_out.value
    assert 0 <= k_out <= n
    used = dict(xo=k_out, co=k_out, pv=n, vc=k_out)
    res = {}
    for k, v in got.items():
        if v is None:
            res[k] = None
            continue
        sent = F_SENT if v.dtype == np.float32 else I_SENT
        assert (v[:GUARD] == sent).all() and (v[GUARD + used[k]:] == sent).all(), f"{k}: written outside rows [0, {used[k]})"
        res[k] = v[GUARD:GUARD + used[k]].copy()
    return rc, res["xo"], res["co"], res["pv"], res["vc"]


def check_against_restatement(ctx, xyz, col, leaf, expected=None, combos=None):
    for with_colour, trace, device in combos or itertools.product((False, True), (False, True), (False, True)):
        c = col if with_colour else None
        exp = expected[with_colour] if expected else vn.voxel_downsample(xyz, leaf, c)
        rc, xo, co, pv, vc = run_guarded(ctx, xyz, c, leaf, trace, device)
        tag = (with_colour, trace, device)
        assert rc == capi.SVO_OK, (tag, ctx.lib.svo_last_error())
        assert xo.shape == exp[0].shape and np.array_equal(bits(xo), bits(exp[0])), tag
        if with_colour:
            assert np.array_equal(bits(co), bits(exp[1])), tag
        if trace:
            assert np.array_equal(pv, exp[2]) and np.array_equal(vc, exp[3]), tag


@pytest.mark.parametrize("name", sorted(vf.FIXTURES))
def test_fixtures_bit_for_bit(ctx, name):
    xyz, col, leaf = vf.build(name)
    check_against_restatement(ctx, xyz, col, leaf, expected={w: vf.expected(name, w)[:4] for w in (False, True)})


@pytest.mark.parametrize("n", vf.SIZES)
def test_sizes_bit_for_bit(ctx, n):
    xyz, col = vf.random_cloud(n, seed=n, bad_every=17 if n > 2 else 0), vf.colours(n, n)
    check_against_restatement(ctx, xyz, col, 0.5)


@pytest.mark.parametrize("n", [64, 65, 4097])
def test_one_voxel_at_the_chunk_seams(ctx, n):
    """the accumulation takes a voxel 64 points at a time: one voxel of exactly one chunk, one past it, and past a radix tile"""
    xyz = np.random.default_rng(n).uniform(0, 0.4, (n, 3)).astype(np.float32)
    exp = vn.voxel_downsample(xyz, 1.0, vf.colours(n, 3))
    assert exp[3].tolist() == [n]
    check_against_restatement(ctx, xyz, vf.colours(n, 3), 1.0, combos=[(True, True, False), (False, True, True)])


def test_more_tiles_than_one_wave_of_the_tile_scan(ctx):
    """64 x 4096 + 1 points, one per voxel along a line: 65 tiles whose head counts are all non-zero, so the scan of the tile counts
    passes a wave's total on to the next wave"""
    n = 64 * 4096 + 1
    xyz = np.zeros((n, 3), np.float32)
    xyz[:, 0] = np.arange(n, dtype=np.float32)
    exp = vn.voxel_downsample(xyz, 1.0)
    assert len(exp[0]) == n and np.array_equal(exp[2], np.arange(n))
    check_against_restatement(ctx, xyz, None, 1.0, expected={False: exp[:4]}, combos=[(False, True, False), (False, False, True)])


def test_wrapper_returns_the_same(ctx):
    import torch

    xyz, col, leaf = vf.build("nonfinite_ends")
    exp = vf.expected("nonfinite_ends")
    a = ctx.voxel_downsample(xyz, leaf, col, trace=True)
    for g, e in zip(a, exp[:4]):
        assert g.dtype == e.dtype and np.array_equal(bits(g), bits(e))
    b = ctx.voxel_downsample(xyz, leaf)
    assert len(b) == 2 and b[1] is None and np.array_equal(bits(b[0]), bits(vf.expected("nonfinite_ends", False)[0]))
    dev = torch.device("cuda", 0)
    d = ctx.voxel_downsample(torch.from_numpy(xyz).to(dev), leaf, torch.from_numpy(col).to(dev), trace=True)
    for g, e in zip(d, exp[:4]):
        assert g.is_cuda and np.array_equal(bits(g.cpu().numpy()), bits(e))
    e0 = ctx.voxel_downsample(np.zeros((0, 3), np.float32), leaf, np.zeros((0, 3), np.float32), trace=True)
    assert [len(x) for x in e0] == [0, 0, 0, 0]


def test_five_runs_are_identical(ctx):
    xyz, col, leaf = vf.build("straddles_tiles")
    runs = [ctx.voxel_downsample(xyz, leaf, col, trace=True) for _ in range(5)]
    for r in runs[1:]:
        assert all(a.tobytes() == b.tobytes() for a, b in zip(r, runs[0]))
    assert runs[0][0].tobytes() == vf.expected("straddles_tiles")[0].tobytes()


def test_two_contexts_take_turns(ctx):
    other = capi.Context(0)
    try:
        names = ["leaf_tenth", "straddles_tiles", "duplicates", "one_voxel"]
        for k, name in enumerate(names + names[::-1]):
            xyz, col, leaf = vf.build(name)
            got = (ctx if k % 2 else other).voxel_downsample(xyz, leaf, col, trace=True)
            assert all(np.array_equal(bits(g), bits(e)) for g, e in zip(got, vf.expected(name)[:4])), (k, name)
    finally:
        other.close()


def test_buffer_reuse_leaves_no_stale_row(ctx):
    """a fresh context called at 8193 points and then at 65: the work buffers are the big call's, no row of it may show"""
    c = capi.Context(0)
    try:
        big, small = vf.random_cloud(8193, seed=8193, bad_every=17), vf.random_cloud(65, seed=65, bad_every=17)
        check_against_restatement(c, big, vf.colours(8193, 1), 0.5, combos=[(True, True, False)])
        check_against_restatement(c, small, vf.colours(65, 2), 0.5, combos=[(True, True, False), (True, True, True), (False, True, False)])
        check_against_restatement(c, big, vf.colours(8193, 1), 0.5, combos=[(False, True, True)])
    finally:
        c.close()


def test_refusals_leave_the_outputs_untouched(ctx):
    xyz, col = vf.random_cloud(100, 1), vf.colours(100, 1)
    for device in (False, True):
        for leaf in (0.0, -1.0, float("nan"), float("inf")):
            assert run_guarded(ctx, xyz, col, leaf, True, device)[0] == capi.SVO_ERR_ARG
        for axis in range(3):   # an axis at 2^21 cells: decided from the bounds the device found, before any key
            edge, leaf = vf.cells_edge(True, axis)
            assert run_guarded(ctx, edge, vf.colours(3, 0), leaf, True, device)[0] == capi.SVO_ERR_CAPACITY
            assert b"too small" in ctx.lib.svo_last_error()
            edge, leaf = vf.cells_edge(False, axis)
            check_against_restatement(ctx, edge, vf.colours(3, 0), leaf, combos=[(True, True, device)])
        # a far outlier makes the leaf too small for the cloud; the same cloud with the outlier non-finite is fine
        far = xyz.copy()
        far[50] = [3e6, 0, 0]
        assert run_guarded(ctx, far, col, 0.5, True, device)[0] == capi.SVO_ERR_CAPACITY
        far[50, 0] = np.inf
        check_against_restatement(ctx, far, col, 0.5, combos=[(True, True, device)])
    with pytest.raises(capi.SvoError) as e:
        ctx.voxel_downsample(xyz, -0.5)
    assert e.value.code == capi.SVO_ERR_ARG
    n_out = C.c_int(-9)
    rc = ctx.lib.svo_voxel_downsample(ctx._h, None, None, (1 << 22) + 1, C.c_double(0.5), None, None, C.byref(n_out), None, None, capi.MEM_HOST)
    assert rc == capi.SVO_ERR_ARG and n_out.value == -9     # null arrays come first
    one = np.zeros((1, 3), np.float32)
    p = one.ctypes.data_as(C.c_void_p)
    rc = ctx.lib.svo_voxel_downsample(ctx._h, p, None, (1 << 22) + 1, C.c_double(0.5), p, None, C.byref(n_out), None, None, capi.MEM_HOST)
    assert rc == capi.SVO_ERR_CAPACITY and n_out.value == -9 and (one == 0).all()


def test_neighbours_on_the_context_keep_their_bits(ctx):
    rng = np.random.default_rng(4)
    xyz = np.concatenate([icp_fx.corner(4097, step=0.125), (10 + 8 * rng.random((300, 3))).astype(np.float32)])
    sor_a = ctx.sor_filter_large(xyz)
    cl = capi.Cloud(ctx, xyz)
    knn_a = cl.knn(8)
    down_a = ctx.voxel_downsample(xyz, 0.3, trace=True)
    sor_b = ctx.sor_filter_large(xyz)
    knn_b = cl.knn(8)
    down_b = ctx.voxel_downsample(xyz, 0.3, trace=True)
    cl.close()
    assert sor_a[0].tobytes() == sor_b[0].tobytes() and sor_a[2].tobytes() == sor_b[2].tobytes() and 0 < len(sor_a[0]) < len(xyz)
    assert knn_a.tobytes() == knn_b.tobytes()
    exp = vn.voxel_downsample(xyz, 0.3)
    for a, b, e in zip((down_a[0], down_a[2], down_a[3]), (down_b[0], down_b[2], down_b[3]), (exp[0], exp[2], exp[3])):
        assert a.tobytes() == b.tobytes() == e.tobytes()


def test_pose_graph_optimize_with_the_down_sample(ctx):
    """The corner pair through PoseGraphOptimize(voxel_down_sample=True) at downSampleFactor 0.5: the planes' patches lie 2 m from
    each other's planes, and at a 0.5 m voxel a 30-neighbourhood reaches about 1.5 m, so every normal still comes from one plane
    (at 1.0 they would not).  A voxel's mean of points of one plane lies in that plane up to the float rounding of the store,
    2^-21 m at 12 m -- the rounding the pair's tolerance was derived from (tests/test_icp_numpy.py: 1e-5 m, 1e-6 rad)."""
    from scipy.spatial.transform import Rotation as Rot

    c = icp_fx.cases()["corner_pair"]
    f = 0.5
    pgo = registration.PoseGraphOptimize(ctx, downSampleFactor=f, voxel_down_sample=True)
    assert (pgo.max_correspondence_distance_coarse, pgo.max_correspondence_distance_fine) == (7.5, 0.75)
    T, L = pgo.pairwiseRegistration(c["src"], c["tgt"])
    D = T @ np.linalg.inv(icp_fx.known_pose())
    centre = np.r_[c["tgt"].astype(np.float64).mean(0), 1.0]
    dt = np.linalg.norm((D @ centre - centre)[:3])
    dr = np.linalg.norm(Rot.from_matrix(D[:3, :3]).as_rotvec())
    print(f"down-sampled corner pair: translation error at the cloud's centre {dt:.2e} m, rotation error {dr:.2e} rad")
    assert dt <= 1e-5 and dr <= 1e-6
    # the same by hand: the down-sample, then the unchanged class
    src = ctx.voxel_downsample(c["src"], f)[0]
    tgt = ctx.voxel_downsample(c["tgt"], f)[0]
    assert 0 < len(src) < len(c["src"]) and 0 < len(tgt) < len(c["tgt"])
    plain = registration.PoseGraphOptimize(ctx, downSampleFactor=f)
    T2, L2 = plain.pairwiseRegistration(src, tgt)
    assert T.tobytes() == T2.tobytes() and L.tobytes() == L2.tobytes()
    # a capi.Cloud target is taken as given; the default leaves the arrays alone
    cl = capi.Cloud(ctx, c["tgt"]).estimate_normals(30)
    T3, _ = pgo.pairwiseRegistration(c["src"], cl)
    T4, _ = plain.pairwiseRegistration(src, cl)
    cl.close()
    assert T3.tobytes() == T4.tobytes()
    # addPoseToGraph with a given pose takes the information of the thinned clouds too
    pgo.poseGraph.augment_node(np.array([0, 0, 1.0, 0, 0, 0, 1]))
    plain.poseGraph.augment_node(np.array([0, 0, 1.0, 0, 0, 0, 1]))
    K = icp_fx.known_pose()
    a = pgo.addPoseToGraph(c["src"], c["tgt"], R=K[:3, :3], t=K[:3, 3], loopClosureNode=0)
    b = plain.addPoseToGraph(src, tgt, R=K[:3, :3], t=K[:3, 3], loopClosureNode=0)
    assert a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()


def pcl_frame(xyz, bgr):
    """pclPublish's conversion: (x, z, y) x 5 in float, colours r, g, b as uint8_t fields hold them"""
    xyz = np.asarray(xyz, np.float32)
    five = np.float32(5)
    p = np.stack([xyz[:, 0] * five, xyz[:, 2] * five, xyz[:, 1] * five], 1)
    c = np.nan_to_num(np.asarray(bgr, np.float32)[:, ::-1], nan=0.0)
    return p, np.trunc(np.clip(c, 0, 255)).astype(np.float32)


def test_adaptor_equals_the_python_path(tmp_path, ctx):
    rng = np.random.default_rng(9)
    xyz = np.concatenate([icp_fx.corner(3000, step=0.125), (10 + 8 * rng.random((200, 3))).astype(np.float32)])
    xyz[7, 1] = np.nan
    bgr = vf.colours(len(xyz), 9)
    (tmp_path / "in.f32").write_bytes(np.concatenate([xyz, bgr], 1).astype(np.float32).tobytes())
    exe = tmp_path / "voxel_smoke"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(ROOT / "tests" / "cpp" / "voxel_smoke.cpp"),
                    f"-L{ROOT / 'ros_stereo_slam_amd'}", "-l:libsvo_hip.so", f"-Wl,-rpath,{ROOT / 'ros_stereo_slam_amd'}",
                    "-o", str(exe)], check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe), str(tmp_path / "in.f32"), str(tmp_path / "o"), "0.3", "1.5"], capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    load = lambda s: np.fromfile(tmp_path / ("o" + s), np.float32).reshape(-1, 3)
    xo, co = ctx.voxel_downsample(xyz, 0.3, bgr)
    assert 0 < len(xo) < len(xyz) and np.array_equal(bits(load(".xyz")), bits(xo)) and np.array_equal(bits(load(".bgr")), bits(co))
    p, c = pcl_frame(xyz, bgr)
    tp, tc = ctx.voxel_downsample(p, 1.5, c)
    xk, ck, _ = ctx.sor_filter_large(tp, tc, mean_k=20, stddev_mul=0.8, z_limit=0.0)
    assert 0 < len(xk) <= len(tp) < len(p)
    assert np.array_equal(bits(load(".pub.xyz")), bits(xk)) and np.array_equal(bits(load(".pub.rgb")), bits(ck))
    xk0, ck0, _ = ctx.sor_filter_large(p, c, mean_k=20, stddev_mul=0.8, z_limit=0.0)
    assert np.array_equal(bits(load(".plain.xyz")), bits(xk0)) and np.array_equal(bits(load(".plain.rgb")), bits(ck0))
