"""The rectification kernels on the GPU, bit for bit against the numpy restatement (tests/rectify_numpy.py): the map build on every
calibration and at the sizes around every seam, the float-map conversion at every boundary, the remap on hand-made maps (no locality,
all outside, every fraction pair) in host and device memory behind guard bands and at every source misalignment, the pair call
against two batch calls at every seam, the composition with the dense matcher, repeatability, two contexts, a map reused after another was destroyed, the known answer on a ramp,
svo_undistort_points, the neighbours on the same context and the refusals."""
import ctypes as C
import itertools
import pathlib
import subprocess

import numpy as np
import pytest

import rectify_fixtures as rf
import rectify_numpy as rn
from ros_stereo_slam_amd import capi

pytestmark = pytest.mark.gpu
GUARD, SENT = 64, 0xA5
ROOT = pathlib.Path(__file__).resolve().parents[1]


def same_map(m, xy, frac):
    gxy, gfr = m.get()
    return gxy.dtype == np.int16 and gfr.dtype == np.uint16 and np.array_equal(gxy, xy) and np.array_equal(gfr, frac)


def test_rig_maps_bit_for_bit(ctx):
    """every calibration at its full size, both cameras, one run"""
    for name in sorted(rf.RIGS):
        K1, D1, K2, D2, size, _, _ = rf.RIGS[name]
        R1, R2, P1, P2, _ = rf.rectification(name)
        for (K, D, R, P), (xy, fr) in zip(((K1, D1, R1, P1), (K2, D2, R2, P2)), rf.rig_maps(name)):
            m = ctx.rectify_map(K, D, R, P, size)
            assert same_map(m, xy, fr), name
            m.close()


@pytest.mark.parametrize("h", rf.HEIGHTS)
def test_map_sizes_bit_for_bit(ctx, h):
    for w in rf.WIDTHS:
        K, D, R, P = rf.tiny_camera(w, h)
        for (Rk, Pk), src in itertools.product(((R, P), (None, None), (R, None), (None, P)), (None, (w + 3, h + 5))):
            m = ctx.rectify_map(K, D, Rk, Pk, (w, h), src_size=src)
            assert m.src_size == (src or (w, h)) and same_map(m, *rn.init_undistort_rectify_map(K, D, Rk, Pk, (w, h))), (w, h, src)
            m.close()


def test_float_maps_bit_for_bit(ctx):
    import torch

    b = rf.BOUNDARY
    mapx, mapy = np.tile(b, (3, 1)), np.tile(b[::-1], (3, 1))
    for w in (1, 3, 4, 5, len(b)):
        mx, my = np.ascontiguousarray(mapx[:, :w]), np.ascontiguousarray(mapy[:, :w])
        exp = rn.float_maps(mx, my)
        for dev in (False, True):
            m = ctx.rectify_map_from_float(*((torch.from_numpy(mx).cuda(), torch.from_numpy(my).cuda()) if dev else (mx, my)), (9, 7))
            assert same_map(m, *exp), (w, dev)
            m.close()
    xy, fr = rf.hand_maps("random", 65, 3, 9, 7, seed=2)
    m = ctx.rectify_map_from_float(*rf.float_of(xy, fr), (9, 7))
    assert same_map(m, xy, fr)
    m.close()


def remap_guarded(ctx, m, src, n, c, value, device, misalign=0):
    """svo_remap_batch with the output between two sentinel bands (and, in device mode, the source `misalign` bytes off a dword)"""
    import torch

    w, h = m.size
    nbytes = n * h * w * c
    if device:
        sbuf = torch.zeros(src.size + 8, dtype=torch.uint8, device="cuda")
        sbuf[misalign:misalign + src.size] = torch.from_numpy(src.reshape(-1)).cuda()
        dbuf = torch.full((nbytes + 2 * GUARD + 8,), SENT, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        sp, dp = sbuf.data_ptr() + misalign, dbuf.data_ptr() + GUARD + misalign
    else:
        s = np.ascontiguousarray(src)
        dbuf = np.full(nbytes + 2 * GUARD + 8, SENT, np.uint8)
        sp, dp = s.ctypes.data, dbuf.ctypes.data + GUARD
        misalign = 0
    rc = ctx.lib.svo_remap_batch(ctx._h, m._h, C.c_void_p(sp), n, c, value, C.c_void_p(dp), capi.MEM_DEVICE if device else capi.MEM_HOST)
    assert rc == capi.SVO_OK, ctx.lib.svo_last_error()
    if device:
        ctx.sync()
        dbuf = dbuf.cpu().numpy()
    lo = GUARD + misalign
    assert (dbuf[:lo] == SENT).all() and (dbuf[lo + nbytes:] == SENT).all(), "written outside the output"
    return dbuf[lo:lo + nbytes].reshape((n, h, w, c) if c == 3 else (n, h, w))


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("h", rf.HEIGHTS)
def test_remap_sizes_bit_for_bit(ctx, h, c):
    sw, sh = 9, 7
    src = np.stack([rf.source(sw, sh, c, 10 + k) for k in range(2)])
    for w in rf.WIDTHS:
        xy, fr = rf.hand_maps("random", w, h, sw, sh, seed=w)
        m = ctx.rectify_map_from_float(*rf.float_of(xy, fr), (sw, sh))
        exp = np.stack([rn.remap(s, xy, fr, 7) for s in src])
        for device in (False, True):
            assert np.array_equal(remap_guarded(ctx, m, src, 2, c, 7, device, misalign=w % 4), exp), (w, h, c, device)
        m.close()


@pytest.mark.parametrize("name", rf.HAND_MAPS)
def test_remap_hand_maps_bit_for_bit(ctx, name):
    for (sw, sh), c in itertools.product(((9, 7), (1, 1), (2, 2)), (1, 3)):
        w, h = (32, 32) if name == "fractions" else (37, 5)
        if name == "identity":
            w, h = sw, sh
        xy, fr = rf.hand_maps(name, w, h, sw, sh, seed=4)
        m = ctx.rectify_map_from_float(*rf.float_of(xy, fr), (sw, sh))
        for n, value in ((1, 0), (2, 7), (16, 255)):
            src = np.stack([rf.source(sw, sh, c, 20 + k) for k in range(n)])
            exp = np.stack([rn.remap(s, xy, fr, value) for s in src])
            if name == "identity":
                assert np.array_equal(exp, src)
            if name == "outside":
                assert (exp == value).all()
            for device, mis in ((False, 0), (True, 0), (True, 1), (True, 2), (True, 3)):
                assert np.array_equal(remap_guarded(ctx, m, src, n, c, value, device, mis), exp), (name, sw, sh, c, n, device, mis)
        m.close()


def test_pairs_repeats_contexts_and_reuse(ctx):
    import torch

    (xl, fl), (xr, fr) = rf.rig_maps("vertical")
    K1, D1, K2, D2, size, _, _ = rf.RIGS["vertical"]
    R1, R2, P1, P2, _ = rf.rectification("vertical")
    other = capi.Context(0)
    try:
        doomed = ctx.rectify_map(K1, D1, None, None, size)
        ml, mr = ctx.rectify_map(K1, D1, R1, P1, size), ctx.rectify_map(K2, D2, R2, P2, size)
        ol = other.rectify_map(K1, D1, R1, P1, size)
        doomed.close()
        for c in (1, 3):
            L = np.stack([rf.source(size[0], size[1], c, 30 + k) for k in range(3)])
            Rr = np.stack([rf.source(size[0], size[1], c, 40 + k) for k in range(3)])
            expL = np.stack([rn.remap(s, xl, fl, 9) for s in L])
            expR = np.stack([rn.remap(s, xr, fr, 9) for s in Rr])
            runs = [ctx.rectify_pairs(ml, mr, L, Rr, border_value=9) for _ in range(5)]
            for a, b in runs:
                assert np.array_equal(a, expL) and np.array_equal(b, expR)
            assert np.array_equal(ctx.remap(ml, L, 9), expL) and np.array_equal(ctx.remap(mr, Rr, 9), expR)
            dl, dr = ctx.rectify_pairs(ml, mr, torch.from_numpy(L).cuda(), torch.from_numpy(Rr).cuda(), border_value=9)
            ctx.sync()
            assert np.array_equal(dl.cpu().numpy(), expL) and np.array_equal(dr.cpu().numpy(), expR)
            for k in range(4):   # two contexts taking turns
                assert np.array_equal((ctx if k % 2 else other).remap(ml if k % 2 else ol, L[k % 3], 9), expL[k % 3])
        assert np.array_equal(ctx.remap(ml, L[0][..., 0] if L[0].ndim == 3 else L[0], 9).shape, (size[1], size[0]))
    finally:
        other.close()


def test_known_answer_on_a_ramp(ctx):
    """The integer-rounded ramp 0.25 x + 0.25 y + 20 through the EuRoC-like map: wherever the four taps are inside (and hold the
    ramp itself: it passes 255 in the far corner, where the uint8 source saturates) the result is within 2 grey levels of the ramp
    at the unrounded (u, v).  Derived: 0.5 (output rounding) + 0.5 (source rounding under convex weights) + (1/64)(0.25 + 0.25)
    (map quantisation) < 1.01, against an integer comparison."""
    K1, D1, _, _, size, _, _ = rf.RIGS["euroc"]
    R1, _, P1, _, _ = rf.rectification("euroc")
    src, f = rf.ramp(*size)
    m = ctx.rectify_map(K1, D1, R1, P1, size)
    out = ctx.remap(m, src).astype(np.float64)
    xy, _ = m.get()
    u, v = rn.rectify_uv(K1, D1, R1, P1, size)
    ok = (rn.taps_outside(xy, size) == 0) & (f(xy[..., 0] + 1.0, xy[..., 1] + 1.0) <= 255)
    err = np.abs(out - f(u, v))[ok]
    print(f"ramp: {ok.sum()} of {ok.size} pixels checked, worst error {err.max():.4f} grey levels")
    assert ok.mean() > 0.5 and err.max() <= 2
    m.close()


def test_undistort_points(ctx):
    import torch

    K, D, _, _, size, _, _ = rf.RIGS["euroc"]
    R1, _, P1, _, _ = rf.rectification("euroc")
    for n in (0, 1, 63, 64, 65, 255, 256, 257):
        pts = (np.random.default_rng(n).uniform(-20, 780, (n, 2))).astype(np.float32)
        for R, P in ((R1, P1), (None, None)):
            exp = rn.undistort_points(pts, K, D, R, P)
            assert np.array_equal(capi.undistort_points_host(pts, K, D, R, P).view(np.uint64), exp.view(np.uint64))
            exp32 = exp.astype(np.float32)
            got = ctx.undistort_points(pts, K, D, R, P)
            assert got.shape == (n, 2) and np.array_equal(got.view(np.uint32), exp32.view(np.uint32)), n
            gd = ctx.undistort_points(torch.from_numpy(pts).cuda(), K, D, R, P)
            ctx.sync()
            assert np.array_equal(gd.cpu().numpy().view(np.uint32), exp32.view(np.uint32)), n


def test_neighbours_keep_their_bits(ctx):
    from ros_stereo_slam_amd import synth

    size = (320, 120)
    L, Rr = synth.Scene().stereo(np.eye(3), np.zeros(3), K=(180.0, 180.0, 160.0, 60.0), size=size)[:2]
    pyr = ctx.pyramid(size[0], size[1], L.shape[2] if L.ndim == 3 else 1)
    a_lv = [pyr.build(L).level(l).tobytes() for l in range(3)]
    a_d = ctx.sgbm(L, Rr, num_disparities=32).tobytes()
    K, D, R, P = rf.tiny_camera(*size)
    m = ctx.rectify_map(K, D, R, P, size)
    once = ctx.remap(m, L)
    assert [pyr.build(L).level(l).tobytes() for l in range(3)] == a_lv and ctx.sgbm(L, Rr, num_disparities=32).tobytes() == a_d
    assert np.array_equal(ctx.remap(m, L), once) and np.array_equal(once, rn.remap(L, *m.get()))
    m.close()
    pyr.close()


def test_refusals_leave_the_outputs_untouched(ctx):
    K, D, R, P = rf.tiny_camera(8, 4)
    m = ctx.rectify_map(K, D, R, P, (8, 4))
    m2 = ctx.rectify_map(K, D, R, P, (8, 5))
    src, dst = np.zeros((16, 4, 8, 3), np.uint8), np.full((16, 4, 8, 3), SENT, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for args in ((m._h, p(src), 0, 1, 0, p(dst), 0), (m._h, p(src), 17, 1, 0, p(dst), 0), (m._h, p(src), 1, 2, 0, p(dst), 0),
                 (m._h, p(src), 1, 1, 256, p(dst), 0), (m._h, p(src), 1, 1, -1, p(dst), 0), (m._h, p(src), 1, 1, 0, p(dst), 2),
                 (None, p(src), 1, 1, 0, p(dst), 0), (m._h, None, 1, 1, 0, p(dst), 0), (m._h, p(src), 1, 1, 0, None, 0)):
        assert ctx.lib.svo_remap_batch(ctx._h, *args) == capi.SVO_ERR_ARG and b"svo_remap_batch" in ctx.lib.svo_last_error()
    assert ctx.lib.svo_rectify_pairs(ctx._h, m._h, m2._h, p(src), p(src), 1, 1, 0, p(dst), p(dst), 0) == capi.SVO_ERR_ARG
    assert (dst == SENT).all()
    h = C.c_void_p(0)
    K9, Dn = np.ascontiguousarray(K), np.ascontiguousarray(D, np.float64)
    mk = lambda w, hh, sw, sh, nD=5: ctx.lib.svo_rectify_map_create(ctx._h, p(K9), p(Dn), nD, None, None, w, hh, sw, sh, C.byref(h))
    assert mk(32768, 1, 4, 4) == capi.SVO_ERR_CAPACITY and mk(4, 4, 1, 32768) == capi.SVO_ERR_CAPACITY
    assert mk(0, 4, 4, 4) == capi.SVO_ERR_ARG and mk(4, 4, 4, -1) == capi.SVO_ERR_ARG and mk(4, 4, 4, 4, nD=3) == capi.SVO_ERR_ARG
    assert not h.value
    with pytest.raises(capi.SvoError):
        ctx.rectify_map(K, np.zeros(12), None, None, (8, 4))
    with pytest.raises(capi.SvoError):
        ctx.rectify_map(K, D, np.zeros((3, 3)), None, (8, 4))   # singular P R
    m.close()
    m2.close()


def pairs_guarded(ctx, ml, mr, L, Rr, n, c, value, device, misalign=0):
    """svo_rectify_pairs with each of the two outputs between sentinel bands of its own (device mode: all four pointers `misalign`
    bytes off a dword) -> (out_left, out_right)"""
    import torch

    w, h = ml.size
    nbytes = n * h * w * c
    mk = lambda: np.full(nbytes + 2 * GUARD + 8, SENT, np.uint8)
    if device:
        def put(a):
            t = torch.zeros(a.size + 8, dtype=torch.uint8, device="cuda")
            t[misalign:misalign + a.size] = torch.from_numpy(a.reshape(-1)).cuda()
            return t
        sl, sr = put(L), put(Rr)
        dl, dr = torch.from_numpy(mk()).cuda(), torch.from_numpy(mk()).cuda()
        torch.cuda.synchronize()
        ptrs = [sl.data_ptr() + misalign, sr.data_ptr() + misalign, dl.data_ptr() + GUARD + misalign, dr.data_ptr() + GUARD + misalign]
    else:
        sl, sr, dl, dr, misalign = np.ascontiguousarray(L), np.ascontiguousarray(Rr), mk(), mk(), 0
        ptrs = [sl.ctypes.data, sr.ctypes.data, dl.ctypes.data + GUARD, dr.ctypes.data + GUARD]
    rc = ctx.lib.svo_rectify_pairs(ctx._h, ml._h, mr._h, C.c_void_p(ptrs[0]), C.c_void_p(ptrs[1]), n, c, value, C.c_void_p(ptrs[2]),
                                   C.c_void_p(ptrs[3]), capi.MEM_DEVICE if device else capi.MEM_HOST)
    assert rc == capi.SVO_OK, ctx.lib.svo_last_error()
    outs = []
    if device:
        ctx.sync()
    for d in (dl, dr):
        d = d.cpu().numpy() if device else d
        lo = GUARD + misalign
        assert (d[:lo] == SENT).all() and (d[lo + nbytes:] == SENT).all(), "written outside the output"
        outs.append(d[lo:lo + nbytes].reshape((n, h, w, c) if c == 3 else (n, h, w)))
    return outs


@pytest.mark.parametrize("c", [1, 3])
def test_pairs_equal_two_batch_calls_at_the_seams(ctx, c):
    """svo_rectify_pairs == two svo_remap_batch calls == the restatement at every seam width, 1, 2 and 16 pairs (blockIdx.z up to 31),
    host and device memory, every misalignment"""
    sw, sh = 9, 7
    for w, h in itertools.product(rf.WIDTHS, (1, 3)):
        n = {1: 16, 64: 16, 257: 16, 5: 2}.get(w, 1)
        (xl, fl), (xr, fr) = rf.hand_maps("random", w, h, sw, sh, seed=w), rf.hand_maps("random", w, h, sw, sh, seed=1000 + w)
        ml, mr = ctx.rectify_map_from_float(*rf.float_of(xl, fl), (sw, sh)), ctx.rectify_map_from_float(*rf.float_of(xr, fr), (sw, sh))
        L = np.stack([rf.source(sw, sh, c, 60 + k) for k in range(n)])
        Rr = np.stack([rf.source(sw, sh, c, 80 + k) for k in range(n)])
        expL, expR = np.stack([rn.remap(s, xl, fl, 7) for s in L]), np.stack([rn.remap(s, xr, fr, 7) for s in Rr])
        for device, mis in ((False, 0), (True, 0), (True, w % 4), (True, 3)):
            gl, gr = pairs_guarded(ctx, ml, mr, L, Rr, n, c, 7, device, mis)
            bl, br = remap_guarded(ctx, ml, L, n, c, 7, device, mis), remap_guarded(ctx, mr, Rr, n, c, 7, device, mis)
            assert np.array_equal(gl, bl) and np.array_equal(gr, br), (w, h, n, device, mis)
            assert np.array_equal(gl, expL) and np.array_equal(gr, expR), (w, h, n, device, mis)
        ml.close()
        mr.close()


def test_composition_with_the_dense_matcher(ctx):
    """Render a pair with the rectified cameras, warp it to the raw rig with the restatement's inverse map (CPU), rectify it on the
    GPU, run svo_sgbm_compute: on the pixels valid in both maps the disparities agree with those of the pair that was never warped
    on all but the share the CPU restatement of the same chain leaves (rectify_fixtures.COMPOSE_SHARE, with the command that
    measured it) plus one percentage point.  A wrong map for a camera, R and P paired wrongly or rows off by a pixel would not."""
    K1, D1, K2, D2, size, _, _ = rf.COMPOSE_RIG
    R1, R2, P1, P2, _ = rf.compose_images()[4]
    ml, mr = ctx.rectify_map(K1, D1, R1, P1, size), ctx.rectify_map(K2, D2, R2, P2, size)
    n, share = rf.compose_share(lambda a, b: ctx.rectify_pairs(ml, mr, a, b),
                                lambda a, b: ctx.sgbm(a, b, num_disparities=rf.COMPOSE_NUM_DISPARITIES))
    print(f"compose on the GPU: {n} pixels valid in both maps, agreeing share {share:.4f} (CPU chain: {rf.COMPOSE_SHARE})")
    assert n > 0 and 1 - share <= (1 - rf.COMPOSE_SHARE) + 0.01
    # the control: with the two maps swapped the chain must NOT pass, or the check shows nothing
    _, wrong = rf.compose_share(lambda a, b: ctx.rectify_pairs(mr, ml, a, b),
                                lambda a, b: ctx.sgbm(a, b, num_disparities=rf.COMPOSE_NUM_DISPARITIES))
    print(f"compose with the maps swapped: agreeing share {wrong:.4f}")
    assert 1 - wrong > (1 - rf.COMPOSE_SHARE) + 0.01
    ml.close()
    mr.close()


def test_adaptor_and_sequence_equal_the_python_path(tmp_path, ctx):
    """tests/cpp/rectify_smoke.cpp: RECTIFY_FLAG inside stereoMatch, reprojectDisparity, stereoTriangulate and monocularTriangulate,
    and StereoSequence(rectifier=).load, on the composition rig's raw pair"""
    from ros_stereo_slam_amd import sequence

    K1, D1, K2, D2, size, R, T = rf.COMPOSE_RIG
    _, _, raw_left, raw_right, _ = rf.compose_images()
    sequence.write_image(str(tmp_path / "l_000000.pgm"), raw_left)
    sequence.write_image(str(tmp_path / "r_000000.pgm"), raw_right)
    lp, rp = str(tmp_path / "l_%06d.pgm"), str(tmp_path / "r_%06d.pgm")
    np.concatenate([np.ravel(K1), D1, np.ravel(K2), D2, np.ravel(R), T]).astype(np.float64).tofile(tmp_path / "calib.f64")
    exe = tmp_path / "rectify_smoke"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(ROOT / "tests" / "cpp" / "rectify_smoke.cpp"),
                    f"-L{ROOT / 'ros_stereo_slam_amd'}", "-l:libsvo_hip.so", f"-Wl,-rpath,{ROOT / 'ros_stereo_slam_amd'}",
                    "-o", str(exe)], check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe), lp, rp, str(tmp_path / "calib.f64"), str(tmp_path / "o")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stdout + out.stderr)
    print(out.stdout.strip())
    rect = capi.stereo_rectify(K1, D1, K2, D2, size, R, T)
    assert np.array_equal(np.fromfile(tmp_path / "o.mats", np.float64), np.concatenate([m.ravel() for m in rect]))
    ml, mr = ctx.rectify_map(K1, D1, rect.R1, rect.P1, size), ctx.rectify_map(K2, D2, rect.R2, rect.P2, size)
    bl, br = sequence.StereoSequence(lp, rp).load(0)                       # B,G,R frames as stereoMatch loads them
    assert bl.shape == (size[1], size[0], 3) and np.array_equal(bl[..., 1], raw_left)
    el, er = ctx.rectify_pairs(ml, mr, bl, br)
    sl, sr = sequence.StereoSequence(lp, rp, rectifier=(ml, mr)).load(0)   # the rectifier hook
    assert np.array_equal(sl, el) and np.array_equal(sr, er) and not np.array_equal(el, bl)
    assert np.array_equal(np.fromfile(tmp_path / "o.left", np.uint8), el.ravel())
    assert np.array_equal(np.fromfile(tmp_path / "o.right", np.uint8), er.ravel())
    disp = ctx.sgbm(el, er)
    assert np.array_equal(np.fromfile(tmp_path / "o.disp", np.int16), disp.ravel()) and (disp >= 16).any()
    xyz, bgr = ctx.stereo_reproject(disp, el, rect.Q, disp_scale=1.0 / 16, z_min=0.01, z_max=5.0, flip_y=True)
    assert len(xyz) > 0 and (xyz[:, 2] > 0).all()                          # metric depths in front of the camera
    assert np.array_equal(np.fromfile(tmp_path / "o.xyz", np.float32).reshape(-1, 3), xyz)
    assert np.array_equal(np.fromfile(tmp_path / "o.bgr", np.float32).reshape(-1, 3), bgr)
    pts = np.array([[10, 20], [300.5, 150.25], [158, 101], [0, 199]], np.float32)
    assert np.array_equal(np.fromfile(tmp_path / "o.pts", np.float32).reshape(-1, 2), ctx.undistort_points(pts, K2, D2, rect.R2, rect.P2))
    ml.close()
    mr.close()


def test_grey_batches_keep_their_shape(ctx):
    """a 3-D array whose last two axes are the source size is a grey batch, also when its first two could be an image's"""
    xy, fr = rf.hand_maps("random", 5, 4, 7, 7, seed=1)
    m = ctx.rectify_map_from_float(*rf.float_of(xy, fr), (7, 7))
    batch = np.stack([rf.source(7, 7, 1, k) for k in range(7)])           # (7, 7, 7): n == src_h, h == src_w
    got = ctx.remap(m, batch, 3)
    assert got.shape == (7, 4, 5) and np.array_equal(got, np.stack([rn.remap(s, xy, fr, 3) for s in batch]))
    one = rf.source(7, 7, 3, 9)
    assert np.array_equal(ctx.remap(m, one, 3), rn.remap(one, xy, fr, 3))
    m.close()
