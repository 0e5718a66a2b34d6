"""StereoProcess::pclPublish (src/StereoCV.cpp:275-296) in the C++ adaptor: the entry point declared and exported, the
member bound with the reference's signature in both type builds, the smoke program compiled; on a GPU box the published
cloud equals the Python path (x 5, axes permuted, sor_filter_large with MeanK 20 / StddevMulThresh 0.8)."""
import pathlib
import subprocess

import numpy as np
import pytest

from ros_stereo_slam_amd import capi

ROOT = pathlib.Path(__file__).resolve().parents[1]
REAL_TYPES = ["-DSVO_WITH_OPENCV", "-DSVO_WITH_EIGEN", f"-I{ROOT / 'tests' / 'cpp' / 'stubs'}"]


def test_header_declares_and_library_exports():
    assert "svo_sor_filter_large" in capi.declared_symbols()
    assert hasattr(capi.load(), "svo_sor_filter_large")
    assert hasattr(capi.Context, "sor_filter_large")


@pytest.mark.parametrize("extra", [(), tuple(REAL_TYPES)], ids=["pod", "opencv_eigen"])
def test_adaptor_binds_the_reference_signature(tmp_path, extra):
    tu = tmp_path / "sig.cpp"
    tu.write_text('''
#include "svo_compat/stereoCV.hpp"
using namespace svo_compat;
using std::vector;
int main() {
    void (StereoProcess::*a)(vector<Point3f>&, vector<Point3f>&) = &StereoProcess::pclPublish;   // include/stereoCV.h:59
    vector<Point3f> StereoProcess::*b = &StereoProcess::publishedCloud;
    vector<Point3f> StereoProcess::*c = &StereoProcess::publishedColors;
    (void)a; (void)b; (void)c;
    return 0;
}
''')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", *extra, f"-I{ROOT / 'include'}", str(tu)],
                   check=True, capture_output=True, text=True)


def _build_smoke(exe):
    src = ROOT / "tests" / "cpp" / "stereo_publish_smoke.cpp"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src),
                    f"-L{ROOT / 'ros_stereo_slam_amd'}", "-l:libsvo_hip.so", f"-Wl,-rpath,{ROOT / 'ros_stereo_slam_amd'}",
                    "-o", str(exe)], check=True, capture_output=True, text=True)


def test_publish_smoke_compiles_and_links(tmp_path):
    _build_smoke(tmp_path / "stereo_publish_smoke")


def pcl_frame(xyz, bgr):
    """pclPublish's conversion: (x, z, y) x 5 in float, r = b-g-r's last, colours as uint8_t fields hold them."""
    xyz = np.asarray(xyz, np.float32)
    five = np.float32(5)
    p = np.stack([xyz[:, 0] * five, xyz[:, 2] * five, xyz[:, 1] * five], 1)
    c = np.nan_to_num(np.asarray(bgr, np.float32)[:, ::-1], nan=0.0)
    return p, np.trunc(np.clip(c, 0, 255)).astype(np.float32)


@pytest.mark.gpu
def test_publish_through_the_adaptor(tmp_path, ctx):
    from ros_stereo_slam_amd import synth

    left, right, _ = synth.Scene().stereo(np.eye(3), np.zeros(3), channels=3)
    disp = ctx.sgbm(left, right)
    fx, fy, cx, cy = synth.KITTI_K
    Q = capi.stereo_rectify_q(fx, fy, cx, cy, -0.5707, 1241, 376)
    xyz, bgr = ctx.stereo_reproject(disp, left, Q, disp_scale=1 / 16, z_max=80.0)
    bgr = bgr.copy()
    bgr[:7] = [[-3.0, 300.0, 12.7], [255.9, 0.2, 1e9], [np.nan, 5, 6], [1, 2, 3], [4, 5, 6], [7, 8, 9], [0, 0, 0]]
    assert len(xyz) > 10000
    (tmp_path / "in.f32").write_bytes(np.concatenate([xyz, bgr], 1).astype(np.float32).tobytes())
    exe = tmp_path / "stereo_publish_smoke"
    _build_smoke(exe)
    out = subprocess.run([str(exe), str(tmp_path / "in.f32"), str(tmp_path / "o")], capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    p, c = pcl_frame(xyz, bgr)
    assert c[:3].tolist() == [[12.0, 255.0, 0.0], [255.0, 0.0, 255.0], [6.0, 5.0, 0.0]]
    xk, ck, _ = ctx.sor_filter_large(p, c, mean_k=20, stddev_mul=0.8, z_limit=0.0)
    assert 0 < len(xk) < len(p)
    assert np.array_equal(np.fromfile(tmp_path / "o.xyz", np.float32).reshape(-1, 3), xk)
    assert np.array_equal(np.fromfile(tmp_path / "o.rgb", np.float32).reshape(-1, 3), ck)
