"""The block matcher at the boundary (CPU only; tests/test_gpu_bm.py runs the kernels): declared and exported, the struct's layout
and defaults, every refusal that needs no device with the outputs untouched, the adaptor's members bound from C++ in both type
builds, the smoke program compiled and linked, and the host decisions of csrc/bm.hip (bm_plan.hip.h) run on their own under the
address and undefined-behaviour sanitizers."""
import ctypes as C
import pathlib
import subprocess

import numpy as np
import pytest

import bm_fixtures as bf
import bm_numpy as bn
from ros_stereo_slam_amd import capi

ROOT = pathlib.Path(__file__).resolve().parents[1]
REAL_TYPES = ["-DSVO_WITH_OPENCV", "-DSVO_WITH_EIGEN", f"-I{ROOT / 'tests' / 'cpp' / 'stubs'}"]
NAMES = ["svo_bm_default_params", "svo_bm_compute", "svo_bm_right_matcher_params", "svo_wls_default_params_bm", "svo_bm_wls_compute",
         "svo_bm_prefilter"]
FIELDS = ["pre_filter_type", "pre_filter_size", "pre_filter_cap", "block_size", "min_disparity", "num_disparities", "texture_threshold",
          "uniqueness_ratio", "speckle_window_size", "speckle_range", "disp12_max_diff"]


def test_header_declares_and_library_exports():
    lib = capi.load()
    for name in NAMES:
        assert name in capi.declared_symbols() and hasattr(lib, name), name
    for name in ("bm", "bm_wls", "bm_prefilter"):
        assert hasattr(capi.Context, name)
    assert callable(capi.bm_params) and callable(capi.bm_right_params) and callable(capi.wls_params_bm)
    text = (ROOT / "include" / "svo.h").read_text()
    assert "SVO_BM_PREFILTER_NORMALIZED_RESPONSE = 0, SVO_BM_PREFILTER_XSOBEL = 1" in text
    assert (capi.BM_PREFILTER_NORMALIZED_RESPONSE, capi.BM_PREFILTER_XSOBEL) == (0, 1)


def test_struct_layout_and_defaults():
    assert [n for n, _ in capi.BmParams._fields_] == FIELDS and C.sizeof(capi.BmParams) == 44
    p = capi.bm_params()
    assert [getattr(p, n) for n in FIELDS] == [1, 9, 31, 21, 0, 64, 10, 15, 0, 0, -1]
    import dataclasses
    assert [getattr(p, n) for n in FIELDS] == list(dataclasses.astuple(bn.Params()))
    capi.load().svo_bm_default_params(None)       # a null pointer is ignored
    q = capi.bm_params(min_disparity=1, num_disparities=96, block_size=15, disp12_max_diff=2, speckle_window_size=9, speckle_range=3)
    r, e = capi.bm_right_params(q), bn.right_matcher_params(bn.Params(**{n: getattr(q, n) for n in FIELDS}))
    assert [getattr(r, n) for n in FIELDS] == [getattr(e, n) for n in FIELDS]
    for b in (5, 7, 15, 21, 31, 101, 255):
        for minD in (-20, 0, 1):
            bp = capi.bm_params(block_size=b, min_disparity=minD, num_disparities=32)
            w, e = capi.wls_params_bm(bp), bn.wls_default_params(bn.Params(block_size=b, min_disparity=minD, num_disparities=32))
            assert (w.lambda_, w.sigma_color, w.lrc_thresh, w.use_confidence) == (8000.0, 1.5, 24, 1)
            assert np.float32(w.roll_off) == np.float32(0.001)
            assert (w.depth_discontinuity_radius, w.roi_left, w.roi_right, w.roi_top, w.roi_bottom) == (
                e.depth_discontinuity_radius, e.roi_left, e.roi_right, e.roi_top, e.roi_bottom)
    sg = capi.wls_params(capi.sgbm_params(block_size=7))
    assert sg.depth_discontinuity_radius == 4       # the SGBM case keeps ceil(0.5 * block)


def _images(w=64, h=40, c=1, n=1):
    return np.full((n, h, w, c), 7, np.uint8), np.full((n, h, w, c), 9, np.uint8)


def test_every_refusal_without_a_device_leaves_the_outputs_untouched():
    """decided before the context is looked at: a token stands in for it, nothing is launched"""
    lib = capi.load()
    token = C.c_void_p(C.addressof(C.create_string_buffer(64)))

    def refused(code, w=64, h=40, c=1, n=1, ctx=token, mem=capi.MEM_HOST, null=None, **over):
        prm = capi.bm_params(**over)
        L, R = _images()
        out = np.full((16, 40, 64), -77, np.int16)
        args = dict(left=capi._ptr(L), right=capi._ptr(R), disp=capi._ptr(out))
        if null:
            args[null] = None
        rc = lib.svo_bm_compute(ctx, C.byref(prm) if null != "prm" else None, args["left"], args["right"], w, h, c, n, args["disp"], mem)
        assert rc == code and lib.svo_last_error(), (over, rc)
        assert (out == -77).all()
        # the chain refuses the same, with all four outputs untouched
        wp = capi.wls_params_bm(capi.bm_params(), roi_left=0, roi_right=0, roi_top=0, roi_bottom=0)   # the filter's own checks pass
        outs = [np.full((16, 40, 64), -77, np.int16) for _ in range(3)] + [np.full((16, 40, 64), -77, np.float32)]
        rc = lib.svo_bm_wls_compute(ctx, C.byref(prm) if null != "prm" else None, C.byref(wp), args["left"], args["right"], w, h, c, n,
                                    capi._ptr(outs[0]) if null != "disp" else None, capi._ptr(outs[1]), capi._ptr(outs[2]),
                                    capi._ptr(outs[3]), mem)
        assert rc == code and all((o == -77).all() for o in outs), (over, rc)

    A, CAP = capi.SVO_ERR_ARG, capi.SVO_ERR_CAPACITY
    for n in (0, -1, 17):
        refused(A, n=n)
    for c in (0, 2, 4):
        refused(A, c=c)
    for nd in (0, -16, 8, 24, 272):
        refused(A, num_disparities=nd)
    for b in (3, 4, 20, 256, 257, -5):
        refused(A, block_size=b)
    refused(A, block_size=41)                         # above min(w, h) = 40
    refused(A, w=20, h=40)                            # the default block of 21 above w
    for cap in (0, 64, -3):
        refused(A, pre_filter_cap=cap)
    for s in (3, 4, 10, 257):
        refused(A, pre_filter_size=s)
    for t in (capi.BM_PREFILTER_NORMALIZED_RESPONSE, 2, -1):
        refused(A, pre_filter_type=t)
    refused(A, texture_threshold=-1)
    refused(A, uniqueness_ratio=-1)
    refused(A, min_disparity=2 ** 30)
    for mem in (-1, 2):
        refused(A, mem=mem)
    for null in ("prm", "left", "right", "disp"):
        refused(A, null=null)
    refused(A, ctx=None)
    refused(CAP, block_size=33)                       # above the plan's cap of 31 (w, h = 64, 40 allow it)
    refused(CAP, w=2049, h=40)
    refused(CAP, w=2048, h=128, n=16, num_disparities=256, block_size=5)
    assert bf.plan_constants()["MAX_BLOCK"] == 31

    # svo_bm_prefilter
    img, out = np.full((8, 8), 3, np.uint8), np.full((8, 8), 99, np.uint8)
    for kw in (dict(c=2), dict(cap=0), dict(cap=64), dict(w=0), dict(h=0), dict(mem=5), dict(ctx=None)):
        a = dict(ctx=token, w=8, h=8, c=1, cap=31, mem=capi.MEM_HOST)
        a.update(kw)
        assert lib.svo_bm_prefilter(a["ctx"], capi._ptr(img), a["w"], a["h"], a["c"], a["cap"], capi._ptr(out), a["mem"]) == A, kw
    assert lib.svo_bm_prefilter(token, capi._ptr(img), 2049, 8, 1, 31, capi._ptr(out), capi.MEM_HOST) == CAP
    assert (out == 99).all()


@pytest.mark.parametrize("extra", [(), tuple(REAL_TYPES)], ids=["pod", "opencv_eigen"])
def test_signatures_bind(tmp_path, extra):
    tu = tmp_path / "sig.cpp"
    tu.write_text('''
#include "svo_compat/stereoCV.hpp"
int main() {
    void (*a)(svo_bm_params*) = &svo_bm_default_params;
    int (*b)(svo_ctx*, const svo_bm_params*, const uint8_t*, const uint8_t*, int, int, int, int, int16_t*, int) = &svo_bm_compute;
    void (*c)(const svo_bm_params*, svo_bm_params*) = &svo_bm_right_matcher_params;
    void (*d)(const svo_bm_params*, svo_wls_params*) = &svo_wls_default_params_bm;
    int (*e)(svo_ctx*, const svo_bm_params*, const svo_wls_params*, const uint8_t*, const uint8_t*, int, int, int, int, int16_t*,
             int16_t*, int16_t*, float*, int) = &svo_bm_wls_compute;
    int (*f)(svo_ctx*, const uint8_t*, int, int, int, int, uint8_t*, int) = &svo_bm_prefilter;
    (void)a; (void)b; (void)c; (void)d; (void)e; (void)f;
    static_assert(sizeof(svo_bm_params) == 44, "eleven ints");
    static_assert(SVO_BM_PREFILTER_NORMALIZED_RESPONSE == 0 && SVO_BM_PREFILTER_XSOBEL == 1, "cv::StereoBM's values");
    using namespace svo_compat;
    bool StereoProcess::*flag = &StereoProcess::BM_FLAG;
    svo_bm_params StereoProcess::*prm = &StereoProcess::bmParams;
    bool StereoProcess::*wls = &StereoProcess::WLS_FLAG;                 // unchanged
    Mat (StereoProcess::*m)(int) = &StereoProcess::stereoMatch;          // unchanged
    (void)flag; (void)prm; (void)wls; (void)m;
    return 0;
}
''')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", *extra, f"-I{ROOT / 'include'}", str(tu)],
                   check=True, capture_output=True, text=True)


def build_smoke(exe, extra=()):
    src = ROOT / "tests" / "cpp" / "bm_smoke.cpp"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *extra, f"-I{ROOT / 'include'}", str(src),
                    f"-L{ROOT / 'ros_stereo_slam_amd'}", "-l:libsvo_hip.so", f"-Wl,-rpath,{ROOT / 'ros_stereo_slam_amd'}",
                    "-o", str(exe)], check=True, capture_output=True, text=True)


@pytest.mark.parametrize("extra", [(), tuple(REAL_TYPES)], ids=["pod", "opencv_eigen"])
def test_bm_smoke_compiles_and_links(tmp_path, extra):
    build_smoke(tmp_path / "bm_smoke", extra)


def test_the_flag_defaults_to_off():
    text = (ROOT / "include" / "svo_compat" / "stereoCV.hpp").read_text()
    assert "bool BM_FLAG = false;" in text and "if (BM_FLAG) {" in text


def test_host_decisions_under_the_sanitizers(tmp_path):
    """Every refusal, the geometry, the tile and its LDS layout for every legal (D, block), the scratch layout at its corners, as a
    stand-alone program built with -fsanitize=address,undefined; its tile table is the one bm_fixtures restates."""
    exe = tmp_path / "bm_plan_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{ROOT / 'include'}", str(ROOT / "tests" / "cpp" / "bm_plan_check.cpp"), "-o", str(exe)], check=True,
                   capture_output=True, text=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "bm plan check ok" in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
    rows = [tuple(int(v) for v in line.split()[1:]) for line in out.stdout.splitlines() if line.startswith("tile ")]
    assert len(rows) == 16 * 14
    budget = bf.plan_constants()["LDS_BUDGET"]
    for D, block, tx, total in rows:
        assert bf.tile_width(D, block) == tx and bf.lds_bytes(tx, D, block) == total <= budget <= 160 * 1024, (D, block)
    assert {tx for _, _, tx, _ in rows} >= {64, 16}     # the seam table meets more than one tile width
