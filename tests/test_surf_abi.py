"""svo_surf_* at the boundary: declared and exported, the parameter struct's size and defaults, svo_surf_layers_layout against the
restatement, the signatures of include/svo.h and the adaptor members bound from C++ in both type builds of the compatibility
headers, the flags off by default, the smoke program compiled and linked (CPU only; tests/test_gpu_surf.py runs the program
against the Python path)."""
import ctypes as C
import pathlib
import subprocess

import pytest

import surf_numpy as sn
from ros_stereo_slam_amd import capi

ROOT = pathlib.Path(__file__).resolve().parents[1]
REAL_TYPES = ["-DSVO_WITH_OPENCV", "-DSVO_WITH_EIGEN", f"-I{ROOT / 'tests' / 'cpp' / 'stubs'}"]
NAMES = ["svo_surf_default_params", "svo_surf_extract_batch", "svo_surf_describe", "svo_surf_layers", "svo_surf_layers_layout"]


def test_header_declares_and_library_exports():
    lib = capi.load()
    for name in NAMES:
        assert name in capi.declared_symbols()
        assert hasattr(lib, name)
    for m in ("surf_extract", "surf_describe", "surf_layers"):
        assert hasattr(capi.Context, m)
    assert callable(capi.surf_params) and callable(capi.surf_layers_layout)


def test_params_size_and_defaults():
    assert C.sizeof(capi.SurfParams) == 24
    p = capi.surf_params()
    assert (p.hessian_threshold, p.n_octaves, p.n_octave_layers, p.extended, p.upright) == (100.0, 4, 3, 0, 0)
    d = sn.default_params()
    assert all(getattr(p, k) == v for k, v in d.items())
    q = capi.surf_params(hessian_threshold=500, upright=1)
    assert (q.hessian_threshold, q.upright, q.n_octaves) == (500.0, 1, 4)
    capi.load().svo_surf_default_params(None)   # a null pointer is ignored


@pytest.mark.parametrize("w,h", [(1241, 376), (640, 240), (40, 40), (8, 8)])
@pytest.mark.parametrize("no,nl", [(4, 3), (8, 8), (1, 1), (4, 4)])
def test_layers_layout_equals_the_restatement(w, h, no, nl):
    got = capi.surf_layers_layout(w, h, no, nl)
    ref = sn.layers_layout(w, h, no, nl)
    assert len(got[0]) == no * (nl + 2)
    for g, r in zip(got, ref):
        assert g == r


def test_layers_layout_refusals():
    lib = capi.load()
    buf = (C.c_int * 80)(*([-7] * 80))
    for args in ((0, 8, 4, 3), (8, 0, 4, 3), (16385, 8, 4, 3), (8, 8, 0, 3), (8, 8, 9, 3), (8, 8, 4, 0), (8, 8, 4, 9)):
        assert lib.svo_surf_layers_layout(*args, buf, buf, buf, buf) == capi.SVO_ERR_ARG
    assert all(v == -7 for v in buf)
    assert lib.svo_surf_layers_layout(8, 8, 4, 3, None, None, None, None) == capi.SVO_OK


@pytest.mark.parametrize("extra", [(), tuple(REAL_TYPES)], ids=["pod", "opencv_eigen"])
def test_signatures_bind(tmp_path, extra):
    tu = tmp_path / "sig.cpp"
    tu.write_text('''
#include "svo_compat/bundleAdjust.hpp"
#include "svo_compat/visualSLAM.hpp"
int main() {
    void (*d)(svo_surf_params*) = &svo_surf_default_params;
    int (*e)(svo_ctx*, const uint8_t* const*, int, int, int, int, const svo_surf_params*, int, float*, float*, float*, float*, int*, int*,
             float*, int*, int) = &svo_surf_extract_batch;
    int (*c)(svo_ctx*, const uint8_t*, int, int, int, const svo_surf_params*, const float*, const float*, int, float*, float*, uint8_t*,
             int) = &svo_surf_describe;
    int (*l)(svo_ctx*, const uint8_t*, int, int, int, const svo_surf_params*, float*, float*, int) = &svo_surf_layers;
    int (*y)(int, int, int, int, int*, int*, int*, int*) = &svo_surf_layers_layout;
    (void)d; (void)e; (void)c; (void)l; (void)y;
    static_assert(sizeof(svo_surf_params) == 24, "svo_surf_params");
    static_assert(SVO_K_COUNT == 9, "no kernel id is added");
    using namespace svo_compat;
    double visualOdometry::*bl = &visualOdometry::baseline;
    Mat visualOdometry::*k = &visualOdometry::K;
    int visualOdometry::*hs = &visualOdometry::surfHessian;
    void (visualOdometry::*tri)(Mat, Mat, std::vector<Point3f>&, std::vector<Point2f>&) = &visualOdometry::stereoTriangulate;
    void (visualOdometry::*rel)(int, Mat, Mat, Mat&, std::vector<Point2f>&, std::vector<Point3f>&) = &visualOdometry::relocalizeFrames;
    void (visualOdometry::*feat)(const Mat&, std::vector<KeyPoint>&, std::vector<float>&) = &visualOdometry::surfFeatures;
    bool visualSLAM::*flag = &visualSLAM::SURF_FLAG;
    int visualSLAM::*hs2 = &visualSLAM::surfHessian;
    (void)bl; (void)k; (void)hs; (void)tri; (void)rel; (void)feat; (void)flag; (void)hs2;
    visualOdometry vo(nullptr);
    visualSLAM slam(nullptr);
    if (slam.SURF_FLAG || !slam.DENSE_FLAG) return 2;   // off by default
    return vo.baseline == 0.54 && vo.surfHessian == 500 && slam.surfHessian == 1200 ? 0 : 1;
}
''')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", *extra, f"-I{ROOT / 'include'}", str(tu)],
                   check=True, capture_output=True, text=True)


def build_smoke(exe):
    src = ROOT / "tests" / "cpp" / "surf_stereo_smoke.cpp"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src),
                    f"-L{ROOT / 'ros_stereo_slam_amd'}", "-l:libsvo_hip.so", f"-Wl,-rpath,{ROOT / 'ros_stereo_slam_amd'}",
                    "-o", str(exe)], check=True, capture_output=True, text=True)


def test_surf_stereo_smoke_compiles_and_links(tmp_path):
    build_smoke(tmp_path / "surf_stereo_smoke")


def test_surf_stereo_smoke_compiles_against_the_stubs(tmp_path):
    src = ROOT / "tests" / "cpp" / "surf_stereo_smoke.cpp"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", *REAL_TYPES, f"-I{ROOT / 'include'}", str(src)],
                   check=True, capture_output=True, text=True)
