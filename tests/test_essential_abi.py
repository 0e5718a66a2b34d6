"""findEssentialMat / recoverPose and StereoProcess::monocularTriangulate at the boundary: the entry points declared and
exported, the Context methods present, the adaptor member bound with the reference's signature in both type builds, the
smoke program compiled and linked; svo_decompose_essential (host code) against the numpy restatement."""
import pathlib
import subprocess

import numpy as np
import pytest

import essential_numpy as en
from ros_stereo_slam_amd import capi

ROOT = pathlib.Path(__file__).resolve().parents[1]
REAL_TYPES = ["-DSVO_WITH_OPENCV", "-DSVO_WITH_EIGEN", f"-I{ROOT / 'tests' / 'cpp' / 'stubs'}"]
NAMES = ["svo_essential_5pt", "svo_find_essential", "svo_recover_pose", "svo_decompose_essential"]


def test_header_declares_and_library_exports():
    lib = capi.load()
    for name in NAMES:
        assert name in capi.declared_symbols()
        assert hasattr(lib, name)
    for m in ("essential_5pt", "find_essential", "recover_pose"):
        assert hasattr(capi.Context, m)
    assert callable(capi.decompose_essential)


@pytest.mark.parametrize("extra", [(), tuple(REAL_TYPES)], ids=["pod", "opencv_eigen"])
def test_adaptor_binds_the_reference_signature(tmp_path, extra):
    tu = tmp_path / "sig.cpp"
    tu.write_text('''
#include "svo_compat/stereoCV.hpp"
using namespace svo_compat;
using std::vector;
int main() {
    void (StereoProcess::*a)(const Mat&, const Mat&, vector<Point3f>&) = &StereoProcess::monocularTriangulate;  // include/stereoCV.h:66
    Mat (StereoProcess::*b)(const char*, int) = &StereoProcess::getImg;                                         // include/stereoCV.h:60
    (void)a; (void)b;
    return 0;
}
''')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", *extra, f"-I{ROOT / 'include'}", str(tu)],
                   check=True, capture_output=True, text=True)


def build_smoke(exe):
    src = ROOT / "tests" / "cpp" / "mono_triangulate_smoke.cpp"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src),
                    f"-L{ROOT / 'ros_stereo_slam_amd'}", "-l:libsvo_hip.so", f"-Wl,-rpath,{ROOT / 'ros_stereo_slam_amd'}",
                    "-o", str(exe)], check=True, capture_output=True, text=True)


def test_mono_smoke_compiles_and_links(tmp_path):
    build_smoke(tmp_path / "mono_triangulate_smoke")


def test_bad_arguments_are_refused_without_a_device():
    with pytest.raises(capi.SvoError) as e:
        capi.decompose_essential(np.full(9, np.nan))
    assert e.value.code == capi.SVO_ERR_ARG


def test_decompose_essential_matches_the_restatement():
    rng = np.random.default_rng(3)
    for _ in range(200):
        a = rng.normal(size=3)
        th = np.linalg.norm(a)
        k = a / th
        Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
        t = rng.normal(size=3)
        E = en.essential_from_pose(R, t) + rng.normal(size=(3, 3)) * 1e-3  # noisy: distinct singular values
        R1, R2, tt = capi.decompose_essential(E)
        n1, n2, nt = en.decompose(E)
        for Rx in (R1, R2):
            assert abs(np.linalg.det(Rx) - 1) < 1e-12 and np.abs(Rx @ Rx.T - np.eye(3)).max() < 1e-12
        # equal singular values leave U and V free up to a joint rotation; here they are distinct
        assert np.abs(R1 - n1).max() < 1e-9 and np.abs(R2 - n2).max() < 1e-9 and np.abs(tt - nt).max() < 1e-9
