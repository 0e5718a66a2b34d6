"""tests/cpp/closure_measure_smoke.cpp: visualSLAM::getLCMeasurement and globalPoseGraph's MEASURED_LC_FLAG /
INFORMATION_FLAG through the adaptors.  It compiles and links without OpenCV or Eigen and against the stub headers; on a
GPU it measures the closure of the shared image pair and the graph stores what svo_closure_measure returns."""
import pathlib
import subprocess

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
SRC = ROOT / "tests" / "cpp" / "closure_measure_smoke.cpp"
REAL_TYPES = ["-DSVO_WITH_OPENCV", "-DSVO_WITH_EIGEN", f"-I{ROOT / 'tests' / 'cpp' / 'stubs'}"]


def build_smoke(exe, extra=()):
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *extra, f"-I{ROOT / 'include'}", str(SRC),
                    f"-L{ROOT / 'ros_stereo_slam_amd'}", "-l:libsvo_hip.so", f"-Wl,-rpath,{ROOT / 'ros_stereo_slam_amd'}",
                    "-o", str(exe)], check=True, capture_output=True, text=True)


@pytest.mark.parametrize("extra", [(), tuple(REAL_TYPES)], ids=["pod", "opencv_eigen"])
def test_closure_measure_smoke_compiles_and_links(tmp_path, extra):
    build_smoke(tmp_path / "closure_measure_smoke", extra)


def test_new_members_keep_the_reference_defaults(tmp_path):
    """MEASURED_LC_FLAG and INFORMATION_FLAG are off by default (the reference reads neither T nor `information`), the
    information member is the identity, getLCMeasurement has the dump's shape."""
    tu = tmp_path / "members.cpp"
    tu.write_text('''
#include "svo_compat/visualSLAM.hpp"
using namespace svo_compat;
int main() {
    bool globalPoseGraph::*a = &globalPoseGraph::MEASURED_LC_FLAG;
    bool globalPoseGraph::*b = &globalPoseGraph::INFORMATION_FLAG;
    Matrix6d globalPoseGraph::*c = &globalPoseGraph::information;
    bool (visualSLAM::*d)(const visualSLAM::metaData&, const visualSLAM::metaData&) = &visualSLAM::getLCMeasurement;
    Isometry3d visualSLAM::*e = &visualSLAM::lcMeasurementT;
    void (globalPoseGraph::*f)(const Isometry3d&, int) = &globalPoseGraph::addLoopClosure;
    (void)a; (void)b; (void)c; (void)d; (void)e; (void)f;
    Matrix6d I = Matrix6d::Identity();
    for (int r = 0; r < 6; r++)
        for (int k = 0; k < 6; k++)
            if (I(r, k) != (r == k ? 1.0 : 0.0)) return 1;
    svo_closure_params p;
    svo_closure_default_params(&p);
    return p.pnp_iterations == 100 && p.pnp_reproj_err == 0.1 && p.pnp_confidence == 0.999 && p.f_thr == 1.0 && p.seed == 0 ? 0 : 2;
}
''')
    exe = tmp_path / "members"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(tu), f"-L{ROOT / 'ros_stereo_slam_amd'}",
                    "-l:libsvo_hip.so", f"-Wl,-rpath,{ROOT / 'ros_stereo_slam_amd'}", "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    assert subprocess.run([str(exe)], timeout=60).returncode == 0      # host code only: no GPU is touched


@pytest.mark.gpu
def test_closure_measure_smoke_runs_on_gpu(ctx, tmp_path):
    from closure_fixtures import K4, SEED, SIZE, make_pair
    from ros_stereo_slam_amd import capi

    pair = make_pair(ctx)
    exe = tmp_path / "closure_measure_smoke"
    build_smoke(exe)
    pair["newest"].tofile(tmp_path / "newest.bin")
    pair["matched"].tofile(tmp_path / "matched.bin")
    np.ascontiguousarray(np.hstack([pair["xy"], pair["xyz"]]), np.float32).tofile(tmp_path / "points.bin")
    out = subprocess.run([str(exe), str(tmp_path / "newest.bin"), str(tmp_path / "matched.bin"), str(SIZE[0]), str(SIZE[1]),
                          str(tmp_path / "points.bin"), str(len(pair["xy"])), *[repr(k) for k in K4], str(tmp_path / "out.bin")],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "closure measure smoke ok" in out.stdout, (out.returncode, out.stdout, out.stderr)
    got = np.fromfile(tmp_path / "out.bin", np.float64)
    assert SEED == 11                                                   # the smoke's ransacSeed
    rc, meas, ntrk, ninl = ctx.measure_closure(pair["newest"], pair["matched"], pair["xy"], pair["xyz"], K4, seed=SEED)
    assert rc == capi.SVO_OK
    assert np.array_equal(got[:7], [0, 0, 0, 0, 0, 0, 1])               # MEASURED_LC_FLAG off: the identity, T not read
    # the measurement went through Isometry3d and back: rounding of the rotation matrix round trip
    assert np.abs(got[7:14] - meas).max() < 1e-14
    want = np.diag([50.0] * 3 + [200.0] * 3)
    want[0, 4] = want[4, 0] = 3.0
    assert np.array_equal(got[14:35], want[np.triu_indices(6)])
    assert (got[35], got[36]) == (ntrk, ninl)
