"""The dense stereo matcher's C ABI and C++ adaptor (StereoProcess of include/stereoCV.h:32-73): declared, exported,
compiled in both type builds, bound to the reference's exact member signatures; and on a GPU box the reference's
own sequence through the adaptor equals the Python path."""
import pathlib
import subprocess

import numpy as np
import pytest

from ros_stereo_slam_amd import capi

ROOT = pathlib.Path(__file__).resolve().parents[1]
REAL_TYPES = ["-DSVO_WITH_OPENCV", "-DSVO_WITH_EIGEN", f"-I{ROOT / 'tests' / 'cpp' / 'stubs'}"]
NEW = ["svo_sgbm_default_params", "svo_sgbm_compute", "svo_stereo_rectify_q", "svo_stereo_reproject"]


def test_header_declares_and_library_exports():
    names = capi.declared_symbols()
    assert all(n in names for n in NEW)
    lib = capi.load()
    assert all(hasattr(lib, n) for n in NEW)
    text = (ROOT / "include" / "svo.h").read_text()
    assert "SVO_SGBM_MODE_SGBM" in text and "typedef struct svo_sgbm_params" in text


def test_default_params_are_the_references():
    p = capi.sgbm_params()
    assert (p.min_disparity, p.num_disparities, p.block_size, p.p1, p.p2, p.disp12_max_diff, p.pre_filter_cap,
            p.uniqueness_ratio, p.speckle_window_size, p.speckle_range, p.mode) == (1, 96, 7, 24, 96, 0, 60, 0, 3000, 5, 0)


def test_rectify_q_host_only():
    import sgbm_numpy as sn

    for tx in (0.5707, -0.5707, 0.12):
        assert np.array_equal(capi.stereo_rectify_q(718.856, 718.856, 607.1928, 185.2157, tx, 1241, 376),
                              sn.stereo_rectify_q(718.856, 718.856, 607.1928, 185.2157, tx, 1241, 376))
    with pytest.raises(capi.SvoError):
        capi.stereo_rectify_q(718.0, 718.0, 600.0, 180.0, 0.0, 1241, 376)


@pytest.mark.parametrize("extra", [(), tuple(REAL_TYPES)], ids=["pod", "opencv_eigen"])
def test_adaptor_binds_the_reference_signatures(tmp_path, extra):
    tu = tmp_path / "sig.cpp"
    tu.write_text('''
#include "svo_compat/stereoCV.hpp"
using namespace svo_compat;
using std::vector;
int main() {
    Mat (StereoProcess::*a)(int) = &StereoProcess::stereoMatch;                       // include/stereoCV.h:64
    void (StereoProcess::*b)(Mat, vector<Point3f>&, vector<Point3f>&) = &StereoProcess::reprojectDisparity;   // :65
    const char *StereoProcess::*c = &StereoProcess::lFptr;                            // :37
    const char *StereoProcess::*d = &StereoProcess::rFptr;
    Mat StereoProcess::*e = &StereoProcess::lImg;                                     // :50
    Mat StereoProcess::*f = &StereoProcess::rImg;
    Mat StereoProcess::*g = &StereoProcess::K;                                        // :45
    bool StereoProcess::*h = &StereoProcess::metricDisparity;
    void (StereoProcess::*i)(const Mat &, const Mat &, vector<Point3f> &) = &StereoProcess::stereoTriangulate;
    (void)a; (void)b; (void)c; (void)d; (void)e; (void)f; (void)g; (void)h; (void)i;
    StereoProcess *p = nullptr;
    if (p) { StereoProcess q("l_%06d.png", "r_%06d.png"); (void)q; }
    return 0;
}
''')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", *extra, f"-I{ROOT / 'include'}", str(tu)],
                   check=True, capture_output=True, text=True)


def _build_smoke(exe):
    src = ROOT / "tests" / "cpp" / "stereo_smoke.cpp"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src),
                    f"-L{ROOT / 'ros_stereo_slam_amd'}", "-l:libsvo_hip.so", f"-Wl,-rpath,{ROOT / 'ros_stereo_slam_amd'}",
                    "-o", str(exe)], check=True, capture_output=True, text=True)


def test_stereo_smoke_compiles_and_links(tmp_path):
    _build_smoke(tmp_path / "stereo_smoke")


@pytest.mark.gpu
def test_reference_sequence_through_the_adaptor(tmp_path, ctx):
    import sys

    from ros_stereo_slam_amd import synth

    sys.path.insert(0, str(ROOT / "tests"))
    from test_png_decode import write_png

    scene = synth.Scene(colour=True)
    left, right, _ = scene.stereo(np.eye(3), np.zeros(3), size=(400, 120), channels=3)
    for side, img in (("l", left), ("r", right)):
        # PNG holds R,G,B; imread (and the adaptor's loader) gives B,G,R
        (tmp_path / f"{side}_000004.png").write_bytes(write_png(img[..., ::-1].copy(), 2, 8))
    exe = tmp_path / "stereo_smoke"
    _build_smoke(exe)
    out = subprocess.run([str(exe), str(tmp_path / "l_%06d.png"), str(tmp_path / "r_%06d.png"), "4", str(tmp_path / "o")],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    disp = np.fromfile(tmp_path / "o.disp", np.int16).reshape(120, 400)
    assert np.array_equal(disp, ctx.sgbm(left, right))
    sp_fx, sp_c = 7.188560000000e+02, (6.071928000000e+02, 1.852157000000e+02)
    for tag, tx, scale in (("ref", 0.5707, 1.0), ("metric", -0.5707, 1 / 16)):
        Q = capi.stereo_rectify_q(sp_fx, sp_fx, sp_c[0], sp_c[1], tx, 400, 120)
        xyz, bgr = ctx.stereo_reproject(disp, left, Q, disp_scale=scale)
        assert np.array_equal(np.fromfile(tmp_path / f"o_{tag}.xyz", np.float32).reshape(-1, 3), xyz)
        assert np.array_equal(np.fromfile(tmp_path / f"o_{tag}.bgr", np.float32).reshape(-1, 3), bgr)
