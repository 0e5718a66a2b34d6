"""The robust kernels and the pruning of the pose graph at the boundary: declared and exported, the Python wrappers present, the clean
refusal of a null graph, the signatures of include/svo.h and the adaptor's members bound from C++ in both type builds, the smoke program
compiled and linked, and the host arithmetic of the prune (csrc/pg_prune_plan.hip.h: the kernels refused, the edges that go, the
remap, reachability, the capacity and disconnection refusals) run on its own under the address and undefined-behaviour sanitizers.
CPU only; tests/test_gpu_pg_robust.py runs the kernels and the refusals that need a graph."""
import ctypes as C
import pathlib
import subprocess

import pytest

from ros_stereo_slam_amd import capi

ROOT = pathlib.Path(__file__).resolve().parents[1]
REAL_TYPES = ["-DSVO_WITH_OPENCV", "-DSVO_WITH_EIGEN", f"-I{ROOT / 'tests' / 'cpp' / 'stubs'}"]
NAMES = ["svo_pg_set_robust_kernel", "svo_pg_get_robust_kernel", "svo_pg_set_loop_closure_kernel", "svo_pg_edge_residuals",
         "svo_pg_linearization_weights", "svo_pg_prune_edges"]


def test_header_declares_and_library_exports():
    lib = capi.load()
    for name in NAMES:
        assert name in capi.declared_symbols()
        assert hasattr(lib, name)
    text = (ROOT / "include" / "svo.h").read_text()
    for k, name in enumerate(("NONE", "HUBER", "CAUCHY", "DCS", "GEMAN_MCCLURE")):
        assert getattr(capi, "PG_ROBUST_" + name) == k
        assert any(line.split() == ["#define", "SVO_PG_ROBUST_" + name, str(k)] for line in text.splitlines())
    assert "FROM MEMORY, VERIFY" in text
    for m in ("set_robust_kernel", "robust_kernel", "set_loop_closure_kernel", "edge_residuals", "prune_edges"):
        assert callable(getattr(capi.PoseGraph, m))
    from ros_stereo_slam_amd import registration

    assert callable(registration.PoseGraphOptimize.globalOptimize)
    assert lib.svo_version() == 100


def test_null_graph_fails_cleanly_without_a_device():
    lib = capi.load()
    kind, delta, n = C.c_int(-9), C.c_double(-9.0), C.c_int(-9)
    buf = (C.c_double * 4)(7, 7, 7, 7)
    removed = (C.c_int * 4)(7, 7, 7, 7)
    GM = capi.PG_ROBUST_GEMAN_MCCLURE
    assert lib.svo_pg_set_robust_kernel(None, 0, GM, C.c_double(1.0)) == capi.SVO_ERR_ARG
    assert lib.svo_pg_get_robust_kernel(None, 0, C.byref(kind), C.byref(delta)) == capi.SVO_ERR_ARG
    assert lib.svo_pg_set_loop_closure_kernel(None, GM, C.c_double(1.0)) == capi.SVO_ERR_ARG
    assert lib.svo_pg_edge_residuals(None, buf, buf, buf) == capi.SVO_ERR_ARG
    assert lib.svo_pg_linearization_weights(None, buf) == capi.SVO_ERR_ARG
    assert lib.svo_pg_prune_edges(None, C.c_double(0.25), removed, 4, C.byref(n)) == capi.SVO_ERR_ARG
    assert (kind.value, delta.value, n.value) == (-9, -9.0, -9) and list(buf) == [7] * 4 and list(removed) == [7] * 4


@pytest.mark.parametrize("extra", [(), tuple(REAL_TYPES)], ids=["pod", "opencv_eigen"])
def test_signatures_bind(tmp_path, extra):
    tu = tmp_path / "sig.cpp"
    tu.write_text('''
#include "svo_compat/poseGraph.hpp"
int main() {
    int (*a)(svo_posegraph*, int, int, double) = &svo_pg_set_robust_kernel;
    int (*b)(const svo_posegraph*, int, int*, double*) = &svo_pg_get_robust_kernel;
    int (*c)(svo_posegraph*, int, double) = &svo_pg_set_loop_closure_kernel;
    int (*d)(svo_posegraph*, double*, double*, double*) = &svo_pg_edge_residuals;
    int (*e)(svo_posegraph*, double, int*, int, int*) = &svo_pg_prune_edges;
    int (*f)(svo_posegraph*, double*) = &svo_pg_linearization_weights;
    (void)a; (void)b; (void)c; (void)d; (void)e; (void)f;
    static_assert(SVO_PG_ROBUST_NONE == 0 && SVO_PG_ROBUST_HUBER == 1 && SVO_PG_ROBUST_CAUCHY == 2 && SVO_PG_ROBUST_DCS == 3 &&
                  SVO_PG_ROBUST_GEMAN_MCCLURE == 4, "the kinds");
    static_assert(SVO_K_COUNT == 9, "no kernel id was added");
    static_assert(SVO_VERSION == 100, "the version stays");
    using namespace svo_compat;
    void (globalPoseGraph::*m)(int, double) = &globalPoseGraph::setLoopClosureKernel;
    std::vector<int> (globalPoseGraph::*p)(double) = &globalPoseGraph::pruneLoopClosures;
    void (globalPoseGraph::*q)(const Isometry3d&, int) = &globalPoseGraph::addLoopClosure;      // the reference's members stay
    std::vector<Isometry3d> (globalPoseGraph::*r)() = &globalPoseGraph::globalOptimize;
    (void)m; (void)p; (void)q; (void)r;
    return 0;
}
''')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", *extra, f"-I{ROOT / 'include'}", str(tu)],
                   check=True, capture_output=True, text=True)


def build_smoke(exe, extra=()):
    src = ROOT / "tests" / "cpp" / "pg_robust_smoke.cpp"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *extra, f"-I{ROOT / 'include'}", str(src),
                    f"-L{ROOT / 'ros_stereo_slam_amd'}", "-l:libsvo_hip.so", f"-Wl,-rpath,{ROOT / 'ros_stereo_slam_amd'}",
                    "-o", str(exe)], check=True, capture_output=True, text=True)


@pytest.mark.parametrize("extra", [(), tuple(REAL_TYPES)], ids=["pod", "opencv_eigen"])
def test_pg_robust_smoke_compiles_and_links(tmp_path, extra):
    build_smoke(tmp_path / "pg_robust_smoke", extra)


def test_prune_plan_under_the_sanitizers(tmp_path):
    """The refused kernels (unknown kind, a parameter that is zero, negative, infinite or NaN), and the prune: the empty graph, every
    closure removed, the first and the last edge, repeated endpoints, the consecutive-vertex exemption, the strict threshold, the
    capacity refusal and the disconnecting removal, as a stand-alone program built with -fsanitize=address,undefined."""
    exe = tmp_path / "pg_prune_plan_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    str(ROOT / "tests" / "cpp" / "pg_prune_plan_check.cpp"), "-o", str(exe)], check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "pg prune plan check ok" in out.stdout, (out.returncode, out.stdout, out.stderr)


def test_the_plan_header_is_plain_host_code():
    text = (ROOT / "ros_stereo_slam_amd" / "csrc" / "pg_prune_plan.hip.h").read_text()
    assert "hip/hip_runtime" not in text and "__global__" not in text and "__device__" not in text
    assert '#include "pg_prune_plan.hip.h"' in (ROOT / "ros_stereo_slam_amd" / "csrc" / "posegraph.hip").read_text()
