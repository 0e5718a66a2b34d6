"""svo_voxel_downsample and svo_voxel_grid at the boundary: declared and exported, the wrappers present, the clean refusals without a
device and with untouched outputs, svo_voxel_grid against the restatement on both sides of the 2^21 edge, the signatures of
include/svo.h and the adaptor's member and field bound from C++ in both type builds of the compatibility headers, the smoke program
compiled and linked, and the host decisions of csrc/voxel.hip (voxel_plan.hip.h) run on their own under the address and
undefined-behaviour sanitizers (CPU only; tests/test_gpu_voxel.py runs the kernels)."""
import ctypes as C
import inspect
import pathlib
import subprocess

import numpy as np
import pytest

import voxel_fixtures as vf
import voxel_numpy as vn
from ros_stereo_slam_amd import capi, registration

ROOT = pathlib.Path(__file__).resolve().parents[1]
REAL_TYPES = ["-DSVO_WITH_OPENCV", "-DSVO_WITH_EIGEN", f"-I{ROOT / 'tests' / 'cpp' / 'stubs'}"]
NAMES = ["svo_voxel_downsample", "svo_voxel_grid"]


def test_header_declares_and_library_exports():
    lib = capi.load()
    for name in NAMES:
        assert name in capi.declared_symbols()
        assert hasattr(lib, name)
    assert hasattr(capi.Context, "voxel_downsample") and callable(capi.voxel_grid)
    assert lib.svo_version() == 100 and len(capi.declared_symbols()) == len(set(capi.declared_symbols()))
    text = (ROOT / "include" / "svo.h").read_text()
    assert "SVO_K_COUNT = 9" in text and "#define SVO_VERSION 100" in text
    assert inspect.signature(registration.PoseGraphOptimize.__init__).parameters["voxel_down_sample"].default is False
    params = inspect.signature(capi.Context.voxel_downsample).parameters
    assert list(params)[1:] == ["xyz", "voxel_size", "color", "trace", "mem"] and params["trace"].default is False


def _call(lib, ctx, xyz, col, n, leaf, xo, co, n_out, pv, vc, mem):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    return lib.svo_voxel_downsample(ctx, p(xyz), p(col), n, C.c_double(leaf), p(xo), p(co), n_out, p(pv), p(vc), mem)


def test_null_context_fails_cleanly_without_a_device():
    lib = capi.load()
    xyz, col = np.full((4, 3), 7, np.float32), np.full((4, 3), 9, np.float32)
    xo, co = np.full((4, 3), -5, np.float32), np.full((4, 3), -6, np.float32)
    pv, vc, cnt = np.full(4, -7, np.int32), np.full(4, -8, np.int32), (C.c_int * 1)(-9)
    rc = _call(lib, None, xyz, col, 4, 0.5, xo, co, cnt, pv, vc, capi.MEM_HOST)
    assert rc == capi.SVO_ERR_ARG and b"svo_voxel_downsample" in lib.svo_last_error()
    assert (xo == -5).all() and (co == -6).all() and (pv == -7).all() and (vc == -8).all() and cnt[0] == -9
    # n == 0 without a context is still a null context
    assert _call(lib, None, None, None, 0, 0.5, None, None, cnt, None, None, capi.MEM_HOST) == capi.SVO_ERR_ARG and cnt[0] == -9


def test_every_argument_refusal_leaves_the_outputs_untouched():
    """decided before the context is looked at: a token stands in for it, nothing is launched"""
    lib = capi.load()
    token = C.c_void_p(C.addressof(C.create_string_buffer(64)))
    xyz, col = np.full((4, 3), 7, np.float32), np.full((4, 3), 9, np.float32)

    def refused(code=capi.SVO_ERR_ARG, **over):
        a = dict(xyz=xyz, col=col, n=4, leaf=0.5, xo=np.full((4, 3), -5, np.float32), co=np.full((4, 3), -6, np.float32),
                 n_out=(C.c_int * 1)(-9), pv=np.full(4, -7, np.int32), vc=np.full(4, -8, np.int32), mem=capi.MEM_HOST)
        a.update(over)
        rc = _call(lib, token, a["xyz"], a["col"], a["n"], a["leaf"], a["xo"], a["co"], a["n_out"], a["pv"], a["vc"], a["mem"])
        assert rc == code and b"svo_voxel_downsample" in lib.svo_last_error(), (over, rc)
        for name, fill in (("xo", -5), ("co", -6), ("pv", -7), ("vc", -8)):
            assert a[name] is None or (a[name] == fill).all(), (over, name)
        assert a["n_out"] is None or a["n_out"][0] == -9, over

    refused(n=-1)
    refused(n=-(2 ** 31))
    for leaf in (0.0, -0.0, -1.0, -1e-300, float("nan"), float("inf"), float("-inf")):
        refused(leaf=leaf)
    for mem in (-1, 2, 7):
        refused(mem=mem)
    refused(xyz=None)
    refused(xo=None)
    refused(n_out=None)
    refused(co=None)                                   # colours given, nowhere to put them
    refused(code=capi.SVO_ERR_CAPACITY, n=(1 << 22) + 1)  # decided from the count alone: nothing is read


def test_voxel_grid_equals_the_restatement():
    cases = [([-1, 0, 2], [1, 0, 2.5], 0.5), ([0, 0, 0], [0, 0, 0], 0.1), ([-3.5, 2.25, 7], [1, 4, 9], 0.25),
             ([-40, -40, -40], [-0.5, -0.5, -0.5], 1.5), ([0, 0, 0], [0.3, 2.25, 100], 0.1), ([-1e17, 0, 0], [1e17, 0, 0], 1e18),
             ([-3e38, 0, 0], [3e38, 1, 0], 1e-300), ([0, 0, 0], [4.7e18, 4.5e18, 0], 1.0)]
    for axis in range(3):
        cases += [(vf.cells_edge(r, axis)[0].min(0), vf.cells_edge(r, axis)[0].max(0), 1.0) for r in (True, False)]
    for lo, hi, leaf in cases:
        mb, cells, fits = capi.voxel_grid(lo, hi, leaf)
        emb, ecells, efits = vn.voxel_grid(lo, hi, leaf)
        assert np.array_equal(mb.view(np.uint64), emb.view(np.uint64)) and np.array_equal(cells, ecells) and fits == efits, (lo, hi, leaf)
    # both sides of the edge, by value
    for axis in range(3):
        xyz, leaf = vf.cells_edge(True, axis)
        _, cells, fits = capi.voxel_grid(xyz.min(0), xyz.max(0), leaf)
        assert cells[axis] == 1 << 21 and not fits and b"too small" in capi.load().svo_last_error()
        xyz, leaf = vf.cells_edge(False, axis)
        _, cells, fits = capi.voxel_grid(xyz.min(0), xyz.max(0), leaf)
        assert cells[axis] == (1 << 21) - 1 and fits


def test_voxel_grid_refusals_write_nothing():
    lib = capi.load()
    lo, hi = np.zeros(3, np.float32), np.ones(3, np.float32)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def refused(lo=lo, hi=hi, leaf=1.0, mb=True, cells=True):
        m, c = (np.full(3, 7.0) if mb else None), (np.full(3, 7, np.int64) if cells else None)
        assert lib.svo_voxel_grid(p(lo), p(hi), C.c_double(leaf), p(m), p(c)) == capi.SVO_ERR_ARG
        assert b"svo_voxel_grid" in lib.svo_last_error()
        assert (m is None or (m == 7).all()) and (c is None or (c == 7).all())

    refused(lo=None)
    refused(hi=None)
    refused(mb=False)
    refused(cells=False)
    for leaf in (0.0, -1.0, float("nan"), float("inf")):
        refused(leaf=leaf)
    refused(lo=np.array([0, np.nan, 0], np.float32))
    refused(hi=np.array([1, 1, np.inf], np.float32))
    refused(lo=hi, hi=lo)
    for bad in (0.0, float("nan")):
        with pytest.raises(capi.SvoError):
            capi.voxel_grid(lo, hi, bad)


@pytest.mark.parametrize("extra", [(), tuple(REAL_TYPES)], ids=["pod", "opencv_eigen"])
def test_signatures_bind(tmp_path, extra):
    tu = tmp_path / "sig.cpp"
    tu.write_text('''
#include "svo_compat/stereoCV.hpp"
int main() {
    int (*a)(svo_ctx*, const float*, const float*, int, double, float*, float*, int*, int*, int*, int) = &svo_voxel_downsample;
    int (*b)(const float*, const float*, double, double*, int64_t*) = &svo_voxel_grid;
    (void)a; (void)b;
    static_assert(SVO_K_COUNT == 9, "no kernel id was added");
    static_assert(SVO_VERSION == 100, "the version stays");
    using namespace svo_compat;
    using std::vector;
    void (StereoProcess::*m)(vector<Point3f>&, vector<Point3f>&, double) = &StereoProcess::voxelDownSample;
    double StereoProcess::*f = &StereoProcess::voxelLeaf;
    void (StereoProcess::*p)(vector<Point3f>&, vector<Point3f>&) = &StereoProcess::pclPublish;   // unchanged
    (void)m; (void)f; (void)p;
    return 0;
}
''')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", *extra, f"-I{ROOT / 'include'}", str(tu)],
                   check=True, capture_output=True, text=True)


def build_smoke(exe, extra=()):
    src = ROOT / "tests" / "cpp" / "voxel_smoke.cpp"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *extra, f"-I{ROOT / 'include'}", str(src),
                    f"-L{ROOT / 'ros_stereo_slam_amd'}", "-l:libsvo_hip.so", f"-Wl,-rpath,{ROOT / 'ros_stereo_slam_amd'}",
                    "-o", str(exe)], check=True, capture_output=True, text=True)


@pytest.mark.parametrize("extra", [(), tuple(REAL_TYPES)], ids=["pod", "opencv_eigen"])
def test_voxel_smoke_compiles_and_links(tmp_path, extra):
    build_smoke(tmp_path / "voxel_smoke", extra)


def test_the_field_defaults_to_off():
    text = (ROOT / "include" / "svo_compat" / "stereoCV.hpp").read_text()
    assert "double voxelLeaf = 0;" in text and "if (voxelLeaf > 0 && n > 0)" in text


def test_host_decisions_under_the_sanitizers(tmp_path):
    """The refusals, the grid on both sides of the 2^21 edge and far beyond any integer, the key packing and the buffer layouts up to
    2^22 points, as a stand-alone program built with -fsanitize=address,undefined."""
    exe = tmp_path / "voxel_plan_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    str(ROOT / "tests" / "cpp" / "voxel_plan_check.cpp"), "-o", str(exe)], check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "voxel plan check ok" in out.stdout, (out.returncode, out.stdout, out.stderr)


def test_constants_are_the_kernels():
    plan = (ROOT / "ros_stereo_slam_amd" / "csrc" / "voxel_plan.hip.h").read_text()
    index = (ROOT / "ros_stereo_slam_amd" / "csrc" / "cloud_index.hip.h").read_text()
    assert f"constexpr int TILE = {vf.RS_TILE};" in plan and "RS_THREADS = 256, RS_ROUNDS = 16" in index
    assert "constexpr int64_t MAX_CELLS = 1ll << 21;" in plan and vn.MAX_CELLS == 1 << 21
    assert "constexpr int MAX_POINTS = 1 << 22;" in plan and vn.MAX_POINTS == 1 << 22
    voxel = (ROOT / "ros_stereo_slam_amd" / "csrc" / "voxel.hip").read_text()
    assert '#include "cloud_index.hip.h"' in voxel and "radix_sort_pairs(" in voxel and "radix_scatter_kernel" not in voxel
