"""The disparity WLS filter (svo_wls_filter / svo_sgbm_wls_compute, the calls the reference keeps commented out around its
matcher at src/StereoCV.cpp:25-28,51-59) bit for bit against the numpy restatement tests/wls_numpy.py: the filtered map,
both matchers' raw maps and the confidence plane.  The float order is fixed by W3..W6 and the weight tables come from the
shared svo_exp, so equality is the bound."""
import functools
import pathlib
import subprocess

import numpy as np
import pytest

import sgbm_numpy as sn
import wls_numpy as wn
from ros_stereo_slam_amd import capi, synth

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parents[1]


def _pair(w, h, c=1, shift=7, seed=1, noise=6):
    a, b = synth.textured_pair(w, h, c, shift=(shift, 0), seed=seed, colour=c == 3)
    rng = np.random.default_rng(seed)
    # the left image sees the texture shifted right; a little noise so costs tie rarely but not never
    left = np.clip(b.astype(np.int32) + rng.integers(-noise, noise + 1, b.shape), 0, 255).astype(np.uint8)
    right = np.clip(a.astype(np.int32) + rng.integers(-noise, noise + 1, a.shape), 0, 255).astype(np.uint8)
    return left, right


# name -> (pair arguments, matcher parameters, overrides of the filter's defaults, degenerate)
SMALL = dict(num_disparities=16, block_size=3, speckle_window_size=0)
CASES = {
    "grey_96x40": (dict(w=96, h=40, shift=5, seed=3), SMALL, {}, False),
    "bgr_97x41": (dict(w=97, h=41, c=3, shift=6, seed=4), SMALL, {}, False),
    "min_disparity_-8": (dict(w=160, h=64, shift=4, seed=5), dict(min_disparity=-8, num_disparities=32, block_size=5,
                                                                   speckle_window_size=30), {}, False),
    "roi_width_1": (dict(w=96, h=40, shift=5, seed=3), SMALL, dict(roi_left=50, roi_right=45), True),
    "roi_height_1": (dict(w=96, h=40, shift=5, seed=3), SMALL, dict(roi_top=20, roi_bottom=19), True),
    "no_confidence": (dict(w=96, h=40, shift=5, seed=3), SMALL, dict(use_confidence=0), False),
    "lambda_0": (dict(w=96, h=40, shift=5, seed=3), SMALL, dict(lambda_=0.0), False),
    "reference_400_0.4": (dict(w=131, h=47, c=3, shift=9, seed=6), dict(num_disparities=32, block_size=7, speckle_window_size=50),
                          dict(lambda_=400.0, sigma_color=0.4), False),
    "defaults_8000_1.5": (dict(w=131, h=47, c=3, shift=9, seed=6), dict(num_disparities=32, block_size=7, speckle_window_size=50),
                          {}, False),
    "reference_matcher_640x240": (dict(w=640, h=240, c=3, shift=16, seed=8, noise=4), {}, dict(lambda_=400.0, sigma_color=0.4), False),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """The pair and the restatement's four outputs, computed once and shared (read-only)."""
    pa, mp, over, degenerate = CASES[name]
    left, right = _pair(**pa)
    sp = sn.Params(**mp)
    wp = wn.default_params(sp, **over)
    want = wn.sgbm_wls(left, right, sp, wp)
    for a in (left, right) + tuple(x for x in want if x is not None):
        a.setflags(write=False)
    return left, right, mp, over, wp, want, degenerate


def _assert_meaningful(name):
    """Equality must not be met by an empty result: on the restatement's own output, confidence > 0 on at least half of
    the ROI and the filter changes the map."""
    left, right, mp, over, wp, (out, dl, dr, conf), degenerate = _case(name)
    if degenerate:
        return
    x0, y0, rw, rh = wn.roi(wp, dl.shape[1], dl.shape[0])
    if wp.use_confidence:
        assert (conf[y0:y0 + rh, x0:x0 + rw] > 0).mean() >= 0.5, name
    if wp.lambda_ > 0 or wp.use_confidence:
        assert (out != dl).any(), name


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if not np.array_equal(got.view(np.uint8), np.ascontiguousarray(want).view(np.uint8)):
        bad = np.argwhere(got != want)
        y, x = bad[0][-2:]
        raise AssertionError(f"{what}: {len(bad)} pixels differ, first ({y}, {x}): got {got[y, x]} want {want[y, x]}")


@pytest.mark.parametrize("name", list(CASES))
def test_chain_equals_the_restatement(ctx, name):
    left, right, mp, over, wp, (out, dl, dr, conf), degenerate = _case(name)
    _assert_meaningful(name)
    g_out, g_dl, g_dr, g_conf = ctx.sgbm_wls(left, right, wls=dict(over), want_maps=bool(wp.use_confidence), **mp)
    _same(g_out, out, "filtered")
    _same(g_conf, conf, "confidence")
    if wp.use_confidence:
        _same(g_dl, dl, "left map")
        _same(g_dr, dr, "right map")
    else:
        assert g_dl is None and g_dr is None and not g_conf.any()


def test_right_matcher_alone(ctx):
    """W1: the existing kernels take the right matcher's parameters unchanged."""
    left, right, mp, over, wp, (out, dl, dr, conf), _ = _case("min_disparity_-8")
    rp = capi.sgbm_right_params(capi.sgbm_params(**mp))
    kw = {n: getattr(rp, n) for n, _ in rp._fields_}
    assert kw["min_disparity"] == -23 and kw["disp12_max_diff"] == 1000000
    _same(ctx.sgbm(right, left, **kw), dr, "right map")
    # the right matcher's range is the left one's mirrored: -(minD + numD) + 1 .. -minD, here -23 .. 8
    valid = dr[dr != (kw["min_disparity"] - 1) * 16]
    assert valid.size > dr.size // 2 and valid.min() >= -23 * 16 and valid.max() <= 8 * 16 and (valid < 0).mean() > 0.9


@pytest.mark.parametrize("name", ["bgr_97x41", "no_confidence"])
def test_filter_alone_equals_the_chain(ctx, name):
    left, right, mp, over, wp, (out, dl, dr, conf), _ = _case(name)
    sp = capi.sgbm_params(**mp)
    g_out, g_conf = ctx.wls_filter(dl, dr, sn.cv_gray(left), wls=dict(over), sgbm=sp)
    _same(g_out, out, "filtered")
    _same(g_conf, conf, "confidence")


def test_three_channel_guide(ctx):
    """svo_wls_filter with a BGR guide: the table of the summed squared channel differences."""
    left, right, mp, over, wp, (out, dl, dr, conf), _ = _case("bgr_97x41")
    want, wconf = wn.wls_filter(dl, dr, left, wp)
    assert (want != out).any()   # the colour guide weighs differently from the grey one
    got, gconf = ctx.wls_filter(dl, dr, left, sgbm=capi.sgbm_params(**mp))
    _same(got, want, "filtered")
    _same(gconf, wconf, "confidence")
    again, _ = ctx.wls_filter(dl, dr, sn.cv_gray(left), sgbm=capi.sgbm_params(**mp))   # the table is rebuilt on a change
    _same(again, out, "filtered after a table change")


def test_batch_of_16_equals_its_pairs(ctx):
    pairs = [_pair(96, 40, c=3, shift=3 + k % 5, seed=60 + k) for k in range(16)]
    L = np.stack([p[0] for p in pairs])
    R = np.stack([p[1] for p in pairs])
    batch = ctx.sgbm_wls(L, R, **SMALL)
    assert batch[0].shape == (16, 40, 96)
    for k in range(16):
        one = ctx.sgbm_wls(L[k], R[k], **SMALL)
        for b, o, what in zip(batch, one, ("filtered", "left map", "right map", "confidence")):
            _same(b[k], o, f"pair {k} {what}")
    fb, cb = ctx.wls_filter(batch[1], batch[2], L, sgbm=capi.sgbm_params(**SMALL))
    for k in (0, 7, 15):
        fo, co = ctx.wls_filter(batch[1][k], batch[2][k], L[k], sgbm=capi.sgbm_params(**SMALL))
        _same(fb[k], fo, f"pair {k} filtered (colour guide)")
        _same(cb[k], co, f"pair {k} confidence (colour guide)")
    want = wn.sgbm_wls(L[5], R[5], sn.Params(**SMALL), wn.default_params(sn.Params(**SMALL)))
    for b, o, what in zip(batch, want, ("filtered", "left map", "right map", "confidence")):
        _same(b[5], o, f"pair 5 {what} against the restatement")


def test_device_memory_matches_host(ctx):
    import torch

    left, right, mp, over, wp, want, _ = _case("bgr_97x41")
    dev = ctx.sgbm_wls(torch.from_numpy(left.copy()).cuda(), torch.from_numpy(right.copy()).cuda(), **mp)
    assert all(t.is_cuda for t in dev)
    for t, o, what in zip(dev, want, ("filtered", "left map", "right map", "confidence")):
        _same(t.cpu().numpy(), o, what)
    f, c = ctx.wls_filter(dev[1], dev[2], torch.from_numpy(sn.cv_gray(left).copy()).cuda(), sgbm=capi.sgbm_params(**mp))
    assert f.is_cuda and c.is_cuda
    _same(f.cpu().numpy(), want[0], "filtered")
    _same(c.cpu().numpy(), want[3], "confidence")


BAD_WLS = [dict(lambda_=-1.0), dict(sigma_color=0.0), dict(sigma_color=-2.0), dict(depth_discontinuity_radius=-1),
           dict(roi_left=60, roi_right=36), dict(roi_top=20, roi_bottom=20), dict(roi_left=-1), dict(lambda_=float("nan"))]


@pytest.mark.parametrize("bad", BAD_WLS, ids=[",".join(f"{k}={v}" for k, v in b.items()) for b in BAD_WLS])
def test_refusals_leave_the_outputs_untouched(ctx, bad):
    import ctypes as C

    left, right, mp, over, wp, (out, dl, dr, conf), _ = _case("grey_96x40")
    h, w = dl.shape
    sp = capi.sgbm_params(**mp)
    prm = capi.wls_params(sp, **bad)
    filt, cmap = np.full((h, w), 1234, np.int16), np.full((h, w), 5.5, np.float32)
    m1, m2 = np.full((h, w), 77, np.int16), np.full((h, w), 78, np.int16)
    guide = np.ascontiguousarray(sn.cv_gray(left))
    rc = ctx.lib.svo_wls_filter(ctx._h, C.byref(prm), capi._ptr(dl.copy()), capi._ptr(dr.copy()), capi._ptr(guide), w, h, 1, 1,
                                capi._ptr(filt), capi._ptr(cmap), capi.MEM_HOST)
    assert rc == capi.SVO_ERR_ARG
    rc = ctx.lib.svo_sgbm_wls_compute(ctx._h, C.byref(sp), C.byref(prm), capi._ptr(np.ascontiguousarray(left)),
                                      capi._ptr(np.ascontiguousarray(right)), w, h, 1, 1, capi._ptr(filt), capi._ptr(m1),
                                      capi._ptr(m2), capi._ptr(cmap), capi.MEM_HOST)
    assert rc == capi.SVO_ERR_ARG
    assert (filt == 1234).all() and (cmap == 5.5).all() and (m1 == 77).all() and (m2 == 78).all()


def test_other_refusals(ctx):
    import ctypes as C

    left, right, mp, over, wp, (out, dl, dr, conf), _ = _case("grey_96x40")
    h, w = dl.shape
    sp, prm = capi.sgbm_params(**mp), capi.wls_params(capi.sgbm_params(**mp))
    filt = np.full((h, w), 1234, np.int16)
    guide = np.ascontiguousarray(sn.cv_gray(left))
    args = lambda c, n, right_map: (ctx._h, C.byref(prm), capi._ptr(dl.copy()), capi._ptr(right_map), capi._ptr(guide), w, h, c, n,
                                    capi._ptr(filt), capi._ptr(None), capi.MEM_HOST)
    assert ctx.lib.svo_wls_filter(*args(1, 0, dr.copy())) == capi.SVO_ERR_ARG
    assert ctx.lib.svo_wls_filter(*args(1, 17, dr.copy())) == capi.SVO_ERR_ARG
    assert ctx.lib.svo_wls_filter(*args(2, 1, dr.copy())) == capi.SVO_ERR_ARG
    assert ctx.lib.svo_wls_filter(*args(1, 1, None)) == capi.SVO_ERR_ARG      # use_confidence needs the right map
    # the matcher's own refusals come through the chain, outputs untouched
    bad_sp = capi.sgbm_params(**dict(mp, block_size=4))
    rc = ctx.lib.svo_sgbm_wls_compute(ctx._h, C.byref(bad_sp), C.byref(prm), capi._ptr(np.ascontiguousarray(left)),
                                      capi._ptr(np.ascontiguousarray(right)), w, h, 1, 1, capi._ptr(filt), capi._ptr(None),
                                      capi._ptr(None), capi._ptr(None), capi.MEM_HOST)
    assert rc == capi.SVO_ERR_ARG and (filt == 1234).all()
    with pytest.raises(capi.SvoError):
        ctx.sgbm_wls(left, right, wls=dict(sigma_color=0.0), **mp)
    # and a good call still works afterwards
    _same(ctx.sgbm_wls(left, right, **mp)[0], out, "filtered")


def _build_smoke(exe):
    src = ROOT / "tests" / "cpp" / "wls_smoke.cpp"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src),
                    f"-L{ROOT / 'ros_stereo_slam_amd'}", "-l:libsvo_hip.so", f"-Wl,-rpath,{ROOT / 'ros_stereo_slam_amd'}",
                    "-o", str(exe)], check=True, capture_output=True, text=True)


def test_adaptor_with_wls_flag_equals_the_python_path(tmp_path, ctx):
    import sys

    sys.path.insert(0, str(ROOT / "tests"))
    from test_png_decode import write_png

    scene = synth.Scene(colour=True)
    left, right, _ = scene.stereo(np.eye(3), np.zeros(3), size=(400, 120), channels=3)
    for side, img in (("l", left), ("r", right)):
        # PNG holds R,G,B; imread (and the adaptor's loader) gives B,G,R
        (tmp_path / f"{side}_000004.png").write_bytes(write_png(img[..., ::-1].copy(), 2, 8))
    exe = tmp_path / "wls_smoke"
    _build_smoke(exe)
    out = subprocess.run([str(exe), str(tmp_path / "l_%06d.png"), str(tmp_path / "r_%06d.png"), "4", str(tmp_path / "o")],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    filt, dl, dr, conf = ctx.sgbm_wls(left, right, wls=dict(lambda_=400.0, sigma_color=0.4))
    _same(np.fromfile(tmp_path / "o.raw", np.int16).reshape(120, 400), ctx.sgbm(left, right), "the flag clear: stereoMatch as before")
    _same(np.fromfile(tmp_path / "o.wls", np.int16).reshape(120, 400), filt, "the flag set: filtered map")
    _same(np.fromfile(tmp_path / "o.conf", np.float32).reshape(120, 400), conf, "confidenceMap")
    assert (filt != dl).any() and (conf > 0).mean() > 0.3
