"""svo_fast_* at the boundary: declared and exported, the default parameters, the struct's layout, the clean refusal without a
context, the signatures of include/svo.h and the adaptor's switch bound from C++ in both type builds of the compatibility headers,
the smoke program compiled and linked, and the host arithmetic of csrc/fast.hip (fast_plan.hip.h) run on its own under the address
and undefined-behaviour sanitizers (CPU only; tests/test_gpu_fast.py runs the kernels)."""
import ctypes as C
import pathlib
import subprocess

import numpy as np
import pytest

from ros_stereo_slam_amd import capi

ROOT = pathlib.Path(__file__).resolve().parents[1]
REAL_TYPES = ["-DSVO_WITH_OPENCV", "-DSVO_WITH_EIGEN", f"-I{ROOT / 'tests' / 'cpp' / 'stubs'}"]
NAMES = ["svo_fast_default_params", "svo_fast_detect_batch", "svo_fast_anms_batch"]


def test_header_declares_and_library_exports():
    lib = capi.load()
    for name in NAMES:
        assert name in capi.declared_symbols()
        assert hasattr(lib, name)
    assert "svo_fast_params" in (ROOT / "include" / "svo.h").read_text()       # the fourth symbol of the issue: the struct
    for m in ("fast_detect", "fast_anms"):
        assert hasattr(capi.Context, m)


def test_default_params_and_struct_layout():
    p = capi.fast_params()
    assert (p.threshold, p.nonmax_suppression, p.max_keypoints) == (10, 1, 0)
    assert C.sizeof(capi.FastParams) == 12
    assert [f[0] for f in capi.FastParams._fields_] == ["threshold", "nonmax_suppression", "max_keypoints"]
    assert [getattr(capi.FastParams, f).offset for f in ("threshold", "nonmax_suppression", "max_keypoints")] == [0, 4, 8]
    raw = (C.c_int * 4)(-7, -7, -7, -7)                                          # the call writes three ints and no more
    capi.load().svo_fast_default_params(raw)
    assert list(raw) == [10, 1, 0, -7]
    capi.load().svo_fast_default_params(None)                                    # a null pointer is ignored


def test_null_context_fails_cleanly_without_a_device():
    lib = capi.load()
    img = np.zeros((16, 16), np.uint8)
    ptrs = (C.c_void_p * 1)(img.ctypes.data)
    prm = capi.fast_params()
    xy, resp, n = np.full((8, 2), -1, np.float32), np.full(8, -1, np.float32), (C.c_int * 1)(-9)
    rc = lib.svo_fast_detect_batch(None, ptrs, 1, 16, 16, 1, C.byref(prm), 8, xy.ctypes.data_as(C.c_void_p),
                                   resp.ctypes.data_as(C.c_void_p), None, n, capi.MEM_HOST)
    assert rc == capi.SVO_ERR_ARG and b"svo_fast_detect_batch" in lib.svo_last_error()
    rc = lib.svo_fast_anms_batch(None, ptrs, 1, 16, 16, 1, C.byref(prm), 4, 8, xy.ctypes.data_as(C.c_void_p),
                                 resp.ctypes.data_as(C.c_void_p), n, capi.MEM_HOST)
    assert rc == capi.SVO_ERR_ARG and b"svo_fast_anms_batch" in lib.svo_last_error()
    assert (xy == -1).all() and (resp == -1).all() and n[0] == -9


@pytest.mark.parametrize("extra", [(), tuple(REAL_TYPES)], ids=["pod", "opencv_eigen"])
def test_signatures_bind(tmp_path, extra):
    tu = tmp_path / "sig.cpp"
    tu.write_text('''
#include "svo_compat/visualSLAM.hpp"
int main() {
    void (*d)(svo_fast_params*) = &svo_fast_default_params;
    int (*a)(svo_ctx*, const uint8_t* const*, int, int, int, int, const svo_fast_params*, int, float*, float*, uint8_t*, int*, int) =
        &svo_fast_detect_batch;
    int (*b)(svo_ctx*, const uint8_t* const*, int, int, int, int, const svo_fast_params*, int, int, float*, float*, int*, int) =
        &svo_fast_anms_batch;
    (void)d; (void)a; (void)b;
    static_assert(sizeof(svo_fast_params) == 12, "three ints");
    static_assert(SVO_K_COUNT == 9, "no kernel id was added");
    using namespace svo_compat;
    bool visualSLAM::*flag = &visualSLAM::FAST_FLAG;
    int visualSLAM::*thr = &visualSLAM::fastThreshold;
    int visualSLAM::*keep = &visualSLAM::fastKeep;
    std::vector<KeyPoint> (visualSLAM::*ext)(Mat) = &visualSLAM::fastKeypointExtractor;
    (void)flag; (void)thr; (void)keep; (void)ext;
    return 0;
}
''')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", *extra, f"-I{ROOT / 'include'}", str(tu)],
                   check=True, capture_output=True, text=True)


def test_switch_is_off_by_default(tmp_path):
    tu = tmp_path / "defaults.cpp"
    tu.write_text('''
#include "svo_compat/visualSLAM.hpp"
int main(int argc, char**) {
    if (argc > 1) {            // never taken: the constructor would ask for a device
        svo_compat::visualSLAM v;
        return v.FAST_FLAG || v.fastThreshold != 1 || v.fastKeep != 0 || !v.DENSE_FLAG;
    }
    svo_fast_params p;
    svo_fast_default_params(&p);
    return p.threshold == 10 && p.nonmax_suppression == 1 && p.max_keypoints == 0 ? 0 : 2;
}
''')
    exe = tmp_path / "defaults"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(tu), f"-L{ROOT / 'ros_stereo_slam_amd'}",
                    "-l:libsvo_hip.so", f"-Wl,-rpath,{ROOT / 'ros_stereo_slam_amd'}", "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    assert subprocess.run([str(exe)], timeout=60).returncode == 0      # host code only: no GPU is touched
    text = (ROOT / "include" / "svo_compat" / "visualSLAM.hpp").read_text()
    assert "bool FAST_FLAG = false;" in text and "int fastThreshold = 1;" in text and "int fastKeep = 0;" in text


def build_smoke(exe, extra=()):
    src = ROOT / "tests" / "cpp" / "fast_anms_smoke.cpp"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *extra, f"-I{ROOT / 'include'}", str(src),
                    f"-L{ROOT / 'ros_stereo_slam_amd'}", "-l:libsvo_hip.so", f"-Wl,-rpath,{ROOT / 'ros_stereo_slam_amd'}",
                    "-o", str(exe)], check=True, capture_output=True, text=True)


@pytest.mark.parametrize("extra", [(), tuple(REAL_TYPES)], ids=["pod", "opencv_eigen"])
def test_fast_anms_smoke_compiles_and_links(tmp_path, extra):
    build_smoke(tmp_path / "fast_anms_smoke", extra)


def test_host_arithmetic_under_the_sanitizers(tmp_path):
    """Argument checks, launch geometry, the work-buffer layout up to 16 images of 16384 x 16384 and retainBest's cut, as a
    stand-alone program built with -fsanitize=address,undefined."""
    exe = tmp_path / "fast_plan_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    str(ROOT / "tests" / "cpp" / "fast_plan_check.cpp"), "-o", str(exe)], check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "fast plan check ok" in out.stdout, (out.returncode, out.stdout, out.stderr)
