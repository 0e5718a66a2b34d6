"""svo_bm_compute, svo_bm_prefilter and svo_bm_wls_compute on the GPU, bit for bit against tests/bm_numpy.py: every size of the seam
table, the disparity counts, block sizes, ranges and switches of the recipe, grey and BGR, host and device memory behind
sentinel guard bands, batches; determinism, refusals, the neighbours on the same context, the chain against its parts, and the
adaptor's smoke program against the Python path."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import bm_fixtures as bf
import bm_numpy as bn
from ros_stereo_slam_amd import capi

pytestmark = pytest.mark.gpu

CAP_BLOCK = bf.plan_constants()["MAX_BLOCK"]


@pytest.fixture(scope="module")
def ctx():
    import torch  # noqa: F401  (loads the HIP runtime)

    c = capi.Context(0)
    yield c
    c.close()


def check(ctx, w, h, c=1, shift=4, seed=0, **kw):
    L, R = bf.textured_pair(w, h, c, shift, seed)
    exp = bf.reference(w, h, c, shift, seed, tuple(sorted(kw.items())))
    got = ctx.bm(L, R, **kw)
    assert got.dtype == np.int16 and np.array_equal(got, exp), (w, h, c, kw, int((got != exp).sum()))
    return exp


@pytest.mark.parametrize("h", [1, 2, 7, 8])
@pytest.mark.parametrize("c", [1, 3])
def test_prefilter_equals_the_restatement(ctx, h, c):
    for w, cap in ((3, 31), (17, 1), (131, 31), (300, 63)):
        L, _ = bf.textured_pair(w, h, c, 2, seed=h + w, flat=False)
        exp = bn.prefilter_xsobel(bn.sn.cv_gray(L), cap)
        assert np.array_equal(ctx.bm_prefilter(L, cap), exp), (w, h, c, cap)
        if h % 2:
            assert (exp[-1] == cap).all()


SEAM_PARAMS = [dict(num_disparities=16, block_size=5), dict(num_disparities=64, block_size=21),
               dict(num_disparities=16, block_size=CAP_BLOCK, min_disparity=-3), dict(num_disparities=64, block_size=5, min_disparity=5)]


@pytest.mark.parametrize("kw", SEAM_PARAMS, ids=lambda kw: "-".join(f"{k[:3]}{v}" for k, v in kw.items()))
def test_every_seam_size(ctx, kw):
    sizes = bf.seam_sizes(bn.Params(**kw))
    assert len(sizes) >= 9 and max(w for w, _ in sizes) <= 330
    valid = 0
    for w, h in sizes:
        valid += int((check(ctx, w, h, **kw) != bn.filtered_value(bn.Params(**kw))).sum())
    assert valid > 0


def test_the_tile_shrinks_with_the_disparity_count(ctx):
    assert bf.tile_width(16, 5) == 64 and bf.tile_width(256, CAP_BLOCK) < 64
    kw = dict(num_disparities=256, block_size=CAP_BLOCK)
    exp = check(ctx, 300, 33, shift=9, **kw)          # the one D = 256 case: three tiles of 16 columns, two bands
    assert (exp != -16).any()
    kw = dict(num_disparities=256, block_size=5, uniqueness_ratio=0)
    check(ctx, 300, 12, shift=200, **kw)


@pytest.mark.parametrize("minD", [-3, 0, 5])
@pytest.mark.parametrize("ratio", [0, 15])
def test_ranges_and_switches(ctx, minD, ratio):
    for tex in (0, 10, 4000):
        for d12 in (-1, 0, 2):
            kw = dict(num_disparities=16, block_size=7, min_disparity=minD, uniqueness_ratio=ratio, texture_threshold=tex,
                      disp12_max_diff=d12)
            exp = check(ctx, 97, 37, shift=6, **kw)
            if tex < 4000:
                assert (exp != bn.filtered_value(bn.Params(**kw))).any()


@pytest.mark.parametrize("c", [1, 3])
def test_speckle_and_validation_together(ctx, c):
    base = dict(num_disparities=16, block_size=5, uniqueness_ratio=150, disp12_max_diff=1)
    a = check(ctx, 120, 48, c=c, seed=3, **base)
    b = check(ctx, 120, 48, c=c, seed=3, speckle_window_size=2, speckle_range=1000, **base)
    assert (a != b).any()                              # the filter removed something
    check(ctx, 120, 48, c=c, seed=3, speckle_window_size=30, speckle_range=2, **base)
    check(ctx, 120, 48, c=c, seed=3, speckle_window_size=30, speckle_range=-1, **base)      # B10: off


def test_an_empty_band_and_a_one_column_band(ctx):
    L, R = bf.textured_pair(40, 12, 1, 2, flat=False)
    for kw in (dict(num_disparities=48), dict(num_disparities=16, min_disparity=30), dict(num_disparities=16, min_disparity=-60)):
        kw["block_size"] = 5
        assert bn.empty_band(bn.Params(**kw), 40)
        got = ctx.bm(L, R, **kw)
        assert (got == bn.filtered_value(bn.Params(**kw))).all() and np.array_equal(got, bn.bm(L, R, bn.Params(**kw)))
    check(ctx, 16, 12, num_disparities=16, block_size=5, texture_threshold=0, uniqueness_ratio=0)     # width1 = 1


GUARD = 64


def test_host_and_device_memory_behind_guard_bands(ctx):
    import torch

    w, h, n, kw = 65, 33, 2, dict(num_disparities=16, block_size=7, disp12_max_diff=1, speckle_window_size=4, speckle_range=2)
    pairs = [bf.textured_pair(w, h, 3, 4, seed=k) for k in range(n)]
    L, R = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    exp = np.stack([bn.bm(a, b, bn.Params(**kw)) for a, b in pairs])
    prm = capi.bm_params(**kw)
    # host: the output inside a larger array of sentinels
    buf = np.full(GUARD + exp.size + GUARD, -12345, np.int16)
    out = buf[GUARD:GUARD + exp.size]
    rc = ctx.lib.svo_bm_compute(ctx._h, C.byref(prm), capi._ptr(L), capi._ptr(R), w, h, 3, n, C.c_void_p(out.ctypes.data), capi.MEM_HOST)
    assert rc == 0 and np.array_equal(out.reshape(exp.shape), exp)
    assert (buf[:GUARD] == -12345).all() and (buf[-GUARD:] == -12345).all()
    # device: inputs and output in the middle of guarded tensors
    def guarded(a):
        t = torch.full((GUARD + a.size + GUARD,), 201, dtype=torch.uint8, device="cuda")
        t[GUARD:GUARD + a.size] = torch.from_numpy(a.ravel()).cuda()
        return t
    tl, tr = guarded(L), guarded(R)
    to = torch.full((GUARD + exp.size + GUARD,), -12345, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    rc = ctx.lib.svo_bm_compute(ctx._h, C.byref(prm), C.c_void_p(tl.data_ptr() + GUARD), C.c_void_p(tr.data_ptr() + GUARD), w, h, 3, n,
                                C.c_void_p(to.data_ptr() + 2 * GUARD), capi.MEM_DEVICE)
    assert rc == 0 and ctx.lib.svo_ctx_sync(ctx._h) == 0
    got = to.cpu().numpy()
    assert np.array_equal(got[GUARD:-GUARD].reshape(exp.shape), exp)
    assert (got[:GUARD] == -12345).all() and (got[-GUARD:] == -12345).all()
    for t, a in ((tl, L), (tr, R)):
        g = t.cpu().numpy()
        assert (g[:GUARD] == 201).all() and (g[-GUARD:] == 201).all() and np.array_equal(g[GUARD:-GUARD], a.ravel())
    # the tensor path of the wrapper
    dev = ctx.bm(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda(), **kw)
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), exp)


@pytest.mark.parametrize("n", [1, 2, 16])
def test_batches_equal_the_single_calls(ctx, n):
    w, h, kw = 70, 34, dict(num_disparities=16, block_size=5, disp12_max_diff=0, speckle_window_size=3, speckle_range=1)
    pairs = [bf.textured_pair(w, h, 1, 3 + k % 5, seed=40 + k) for k in range(n)]
    L, R = np.stack([p[0] for p in pairs])[..., None], np.stack([p[1] for p in pairs])[..., None]
    got = ctx.bm(L, R, **kw)
    assert got.shape == (n, h, w)
    for k in (0, n // 2, n - 1):
        single = ctx.bm(*pairs[k], **kw)
        assert np.array_equal(got[k], single) and np.array_equal(single, bn.bm(*pairs[k], bn.Params(**kw)))


def test_repeats_and_two_contexts_agree(ctx):
    L, R = bf.textured_pair(131, 40, 3, 5, seed=9)
    kw = dict(num_disparities=32, block_size=9, disp12_max_diff=1, speckle_window_size=10, speckle_range=2)
    first = ctx.bm(L, R, **kw)
    for _ in range(4):
        assert np.array_equal(ctx.bm(L, R, **kw), first)
    other = capi.Context(0)
    try:
        assert np.array_equal(other.bm(L, R, **kw), first)
    finally:
        other.close()


def test_refusals_leave_the_outputs_untouched(ctx):
    L, R = bf.textured_pair(64, 40, 1, 3)
    for code, kw, n in ((capi.SVO_ERR_ARG, dict(num_disparities=24), 1), (capi.SVO_ERR_ARG, dict(block_size=6), 1),
                        (capi.SVO_ERR_ARG, dict(block_size=41), 1), (capi.SVO_ERR_ARG, dict(pre_filter_type=0), 1),
                        (capi.SVO_ERR_ARG, dict(pre_filter_cap=64), 1), (capi.SVO_ERR_ARG, dict(), 17),
                        (capi.SVO_ERR_CAPACITY, dict(block_size=33), 1)):
        prm = capi.bm_params(**kw)
        out = np.full((40, 64), -77, np.int16)
        assert ctx.lib.svo_bm_compute(ctx._h, C.byref(prm), capi._ptr(L), capi._ptr(R), 64, 40, 1, n, capi._ptr(out), capi.MEM_HOST) == code
        assert (out == -77).all()
        wp = capi.wls_params_bm(capi.bm_params(num_disparities=16, block_size=5))
        outs = [np.full((40, 64), -77, np.int16) for _ in range(3)] + [np.full((40, 64), -77, np.float32)]
        rc = ctx.lib.svo_bm_wls_compute(ctx._h, C.byref(prm), C.byref(wp), capi._ptr(L), capi._ptr(R), 64, 40, 1, n, *map(capi._ptr, outs),
                                        capi.MEM_HOST)
        assert rc == code and all((o == -77).all() for o in outs)
    with pytest.raises(capi.SvoError):
        ctx.bm(L, R, num_disparities=24)


def test_the_neighbours_on_the_context_keep_their_bits(ctx):
    L, R = bf.textured_pair(150, 40, 3, 5, seed=2)
    skw = dict(min_disparity=0, num_disparities=32, speckle_window_size=20)
    before = ctx.sgbm(L, R, **skw)
    sp = capi.sgbm_params(**skw)
    dr = ctx.sgbm(R, L, **{n: getattr(capi.sgbm_right_params(sp), n) for n, _ in capi.SgbmParams._fields_})
    wls_before = ctx.wls_filter(before, dr, L, sgbm=sp)
    ctx.bm(L, R, num_disparities=32, block_size=9, disp12_max_diff=1, speckle_window_size=20, speckle_range=2)
    ctx.bm_wls(L, R, num_disparities=32, block_size=9)
    assert np.array_equal(ctx.sgbm(L, R, **skw), before)
    wls_after = ctx.wls_filter(before, dr, L, sgbm=sp)
    assert np.array_equal(wls_after[0], wls_before[0]) and np.array_equal(wls_after[1], wls_before[1])


@pytest.mark.parametrize("w,h", [(bf.width_for_band(bn.Params(num_disparities=16, block_size=5), 65), 33), (64, 48)])
def test_the_chain_equals_its_parts(ctx, w, h):
    kw = dict(num_disparities=16, block_size=5, speckle_window_size=6, speckle_range=2)
    L, R = bf.textured_pair(w, h, 3, 4, seed=6)
    bp = capi.bm_params(**kw)
    wp = capi.wls_params_bm(bp)
    assert wp.depth_discontinuity_radius == 2
    dl = ctx.bm(L, R, **kw)
    dr = ctx.bm(R, L, params=capi.bm_right_params(bp))
    filt, conf = ctx.wls_filter(dl, dr, bn.sn.cv_gray(L), wls=wp)        # the chain's guide is the grey left image
    assert np.array_equal(dl, bn.bm(L, R, bn.Params(**kw))) and np.array_equal(dr, bn.bm(R, L, bn.right_matcher_params(bn.Params(**kw))))
    got = ctx.bm_wls(L, R, **kw)
    for a, b in zip(got, (filt, dl, dr, conf)):
        assert np.array_equal(a, b)
    e = bn.bm_wls(L, R, bn.Params(**kw))
    assert np.array_equal(got[0], e[0]) and np.array_equal(got[3].view(np.uint32), e[3].view(np.uint32))
    # every optional output NULL in turn
    npix = w * h
    for skip in (1, 2, 3):
        outs = [np.full(npix, -77, np.int16) for _ in range(3)] + [np.full(npix, -77, np.float32)]
        ptrs = [capi._ptr(o) if i != skip else None for i, o in enumerate(outs)]
        assert ctx.lib.svo_bm_wls_compute(ctx._h, C.byref(bp), C.byref(wp), capi._ptr(L), capi._ptr(R), w, h, 3, 1, *ptrs, capi.MEM_HOST) == 0
        for i, (o, ref) in enumerate(zip(outs, (filt, dl, dr, conf))):
            assert (o == -77).all() if i == skip else np.array_equal(o.reshape(h, w), ref), (skip, i)
    import torch
    dev = ctx.bm_wls(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda(), want_maps=False, want_confidence=False, **kw)
    assert dev[1] is None and dev[2] is None and dev[3] is None and np.array_equal(dev[0].cpu().numpy(), filt)


def test_the_adaptor_smoke_program_equals_the_python_path(ctx, tmp_path):
    import test_bm_abi
    from test_png_decode import write_png

    exe = tmp_path / "bm_smoke"
    test_bm_abi.build_smoke(exe)
    w, h = 200, 64
    L, R = bf.textured_pair(w, h, 3, 7, seed=11)
    for side, img in (("l", L), ("r", R)):
        # PNG holds R,G,B; the adaptor's loader gives B,G,R
        (tmp_path / f"{side}_000000.png").write_bytes(write_png(img[..., ::-1].copy(), 2, 8))
    out = subprocess.run([str(exe), str(tmp_path / "l_%06d.png"), str(tmp_path / "r_%06d.png"), "0", str(tmp_path / "o")],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "bm smoke ok: 200 x 64" in out.stdout, (out.returncode, out.stdout, out.stderr)
    kw = dict(min_disparity=1, num_disparities=96, speckle_window_size=3000, speckle_range=5)
    raw = np.fromfile(tmp_path / "o.bm", np.int16).reshape(h, w)
    assert np.array_equal(raw, ctx.bm(L, R, **kw)) and np.array_equal(raw, bn.bm(L, R, bn.Params(**kw)))
    filt, _, _, conf = ctx.bm_wls(L, R, wls=dict(lambda_=400.0, sigma_color=0.4), **kw)
    assert np.array_equal(np.fromfile(tmp_path / "o.wls", np.int16).reshape(h, w), filt)
    assert np.array_equal(np.fromfile(tmp_path / "o.conf", np.float32).reshape(h, w).view(np.uint32), conf.view(np.uint32))
