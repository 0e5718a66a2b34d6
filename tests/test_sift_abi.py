"""svo_sift_* at the boundary: declared and exported, the Context methods present, the signatures of include/svo.h bound from
C++ in both type builds of the compatibility headers, the adaptor's switch bound, the smoke program compiled and linked (CPU only;
tests/test_gpu_sift.py runs the program against the Python path)."""
import ctypes as C
import pathlib
import subprocess

import pytest

from ros_stereo_slam_amd import capi

ROOT = pathlib.Path(__file__).resolve().parents[1]
REAL_TYPES = ["-DSVO_WITH_OPENCV", "-DSVO_WITH_EIGEN", f"-I{ROOT / 'tests' / 'cpp' / 'stubs'}"]
NAMES = ["svo_sift_default_params", "svo_sift_extract_batch", "svo_sift_describe", "svo_sift_pyramid", "svo_sift_pyramid_layout"]


def test_header_declares_and_library_exports():
    lib = capi.load()
    for name in NAMES:
        assert name in capi.declared_symbols()
        assert hasattr(lib, name)
    for m in ("sift_extract", "sift_describe", "sift_pyramid"):
        assert hasattr(capi.Context, m)
    assert capi.MATH_EXP == 5 and capi.MATH_FN["exp"] == 5


def test_default_params_are_sift_create():
    p = capi.sift_params()
    assert (p.n_features, p.n_octave_layers, p.contrast_threshold, p.edge_threshold, p.sigma) == (0, 3, 0.04, 10.0, 1.6)
    assert C.sizeof(capi.SiftParams) == 32
    assert capi.sift_params(n_features=10000).n_features == 10000


def test_pyramid_layout_follows_the_recipe():
    import sift_numpy as sn

    lib = capi.load()
    for w, h in ((1241, 376), (640, 240), (2, 2), (47, 31)):
        no, ow, oh = C.c_int(), (C.c_int * 16)(), (C.c_int * 16)()
        assert lib.svo_sift_pyramid_layout(w, h, 3, C.byref(no), ow, oh) == 0
        assert no.value == sn.n_octaves(w, h) and (ow[0], oh[0]) == (2 * w, 2 * h)
    assert lib.svo_sift_pyramid_layout(1, 40, 3, C.byref(no), ow, oh) == capi.SVO_ERR_ARG


@pytest.mark.parametrize("extra", [(), tuple(REAL_TYPES)], ids=["pod", "opencv_eigen"])
def test_signatures_bind(tmp_path, extra):
    tu = tmp_path / "sig.cpp"
    tu.write_text('''
#include "svo_compat/stereoCV.hpp"
int main() {
    void (*d)(svo_sift_params*) = &svo_sift_default_params;
    int (*e)(svo_ctx*, const uint8_t* const*, int, int, int, int, const svo_sift_params*, int, float*, float*, float*, float*, int*,
             float*, int*, int) = &svo_sift_extract_batch;
    int (*c)(svo_ctx*, const uint8_t*, int, int, int, const svo_sift_params*, const float*, const float*, const float*, const int*,
             int, float*, int) = &svo_sift_describe;
    int (*p)(svo_ctx*, const uint8_t*, int, int, int, const svo_sift_params*, float*, float*, int) = &svo_sift_pyramid;
    int (*l)(int, int, int, int*, int*, int*) = &svo_sift_pyramid_layout;
    (void)d; (void)e; (void)c; (void)p; (void)l;
    using namespace svo_compat;
    bool StereoProcess::*flag = &StereoProcess::SIFT_FLAG;
    void (StereoProcess::*feat)(const Mat&, std::vector<KeyPoint>&, std::vector<float>&, int) = &StereoProcess::siftFeatures;
    void (StereoProcess::*mono)(const Mat&, const Mat&, std::vector<Point3f>&) = &StereoProcess::monocularTriangulate;  // include/stereoCV.h:66
    (void)flag; (void)feat; (void)mono;
    if (StereoProcess(nullptr).SIFT_FLAG) return 2;   // off by default
    svo_sift_params prm{10000, 3, 0.04, 10.0, 1.6};
    static_assert(SVO_MATH_EXP == 5, "math ids");
    return prm.n_features == 10000 ? 0 : 1;
}
''')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", *extra, f"-I{ROOT / 'include'}", str(tu)],
                   check=True, capture_output=True, text=True)


def build_smoke(exe):
    src = ROOT / "tests" / "cpp" / "sift_mono_smoke.cpp"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src),
                    f"-L{ROOT / 'ros_stereo_slam_amd'}", "-l:libsvo_hip.so", f"-Wl,-rpath,{ROOT / 'ros_stereo_slam_amd'}",
                    "-o", str(exe)], check=True, capture_output=True, text=True)


def test_sift_mono_smoke_compiles_and_links(tmp_path):
    build_smoke(tmp_path / "sift_mono_smoke")


def test_sift_mono_smoke_compiles_against_the_stubs(tmp_path):
    src = ROOT / "tests" / "cpp" / "sift_mono_smoke.cpp"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", *REAL_TYPES, f"-I{ROOT / 'include'}", str(src)],
                   check=True, capture_output=True, text=True)
