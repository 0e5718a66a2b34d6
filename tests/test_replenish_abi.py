"""svo_dedup_points and svo_replenish at the boundary: declared and exported, the wrappers and the prototype module present, the clean
refusal without a context, the signatures of include/svo.h and the adaptors' members bound from C++ in both type builds of the
compatibility headers, the smoke program compiled and linked, and the host arithmetic of csrc/replenish.hip (replenish_plan.hip.h) run
on its own under the address and undefined-behaviour sanitizers (CPU only; tests/test_gpu_replenish.py runs the kernels)."""
import ctypes as C
import pathlib
import subprocess

import numpy as np
import pytest

from ros_stereo_slam_amd import capi

ROOT = pathlib.Path(__file__).resolve().parents[1]
REAL_TYPES = ["-DSVO_WITH_OPENCV", "-DSVO_WITH_EIGEN", f"-I{ROOT / 'tests' / 'cpp' / 'stubs'}"]
NAMES = ["svo_dedup_points", "svo_replenish"]


def test_header_declares_and_library_exports():
    lib = capi.load()
    for name in NAMES:
        assert name in capi.declared_symbols()
        assert hasattr(lib, name)
    text = (ROOT / "include" / "svo.h").read_text()
    assert "#define SVO_DEDUP_BOX  0" in text and "#define SVO_DEDUP_DISC 1" in text
    assert (capi.DEDUP_BOX, capi.DEDUP_DISC) == (0, 1)
    for m in ("dedup_points", "replenish"):
        assert hasattr(capi.Context, m)
    assert lib.svo_version() == 100 and len(capi.declared_symbols()) == len(set(capi.declared_symbols()))


def test_prototype_module_keeps_the_prototype_names():
    from ros_stereo_slam_amd import prototype

    for m in ("sparseStereoTriangulate", "trackPointsFrame2Frame", "removeDuplicate", "initializeSequence", "step", "trackSequence"):
        assert callable(getattr(prototype.VisOdometry, m))


def test_null_context_fails_cleanly_without_a_device():
    lib = capi.load()
    ref, new = np.full((4, 2), 7, np.float32), np.full((3, 2), 9, np.float32)
    keep, cnt = np.full(3, 0xAB, np.uint8), (C.c_int * 1)(-9)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = lib.svo_dedup_points(None, p(ref), 4, None, 0, p(new), 3, C.c_double(5.0), 0, p(keep), cnt, capi.MEM_HOST)
    assert rc == capi.SVO_ERR_ARG and b"svo_dedup_points" in lib.svo_last_error()
    assert (keep == 0xAB).all() and cnt[0] == -9
    xy, xyz = np.full((8, 2), 7, np.float32), np.full((8, 3), 7, np.float32)
    new3, Rt = np.full((3, 3), 9, np.float32), np.eye(3, 4)
    outs = (C.c_int * 3)(-9, -9, -9)
    args = (p(new), p(new3), 3, C.c_double(5.0), 0, p(Rt), C.byref(outs, 0), C.byref(outs, 4), C.byref(outs, 8), capi.MEM_HOST)
    rc = lib.svo_replenish(None, p(xy), p(xyz), 4, 8, *args)
    assert rc == capi.SVO_ERR_ARG and b"svo_replenish" in lib.svo_last_error()
    assert (xy == 7).all() and (xyz == 7).all() and list(outs) == [-9, -9, -9]


@pytest.mark.parametrize("extra", [(), tuple(REAL_TYPES)], ids=["pod", "opencv_eigen"])
def test_signatures_bind(tmp_path, extra):
    tu = tmp_path / "sig.cpp"
    tu.write_text('''
#include "svo_compat/visualSLAM.hpp"
#include "svo_compat/bundleAdjust.hpp"
int main() {
    int (*a)(svo_ctx*, const float*, int, const int*, int, const float*, int, double, int, uint8_t*, int*, int) = &svo_dedup_points;
    int (*b)(svo_ctx*, float*, float*, int, int, const float*, const float*, int, double, int, const double*, int*, int*, int*, int) =
        &svo_replenish;
    (void)a; (void)b;
    static_assert(SVO_DEDUP_BOX == 0 && SVO_DEDUP_DISC == 1, "the two modes");
    static_assert(SVO_K_COUNT == 9, "no kernel id was added");
    static_assert(SVO_VERSION == 100, "the version stays");
    using namespace svo_compat;
    std::vector<int> (visualSLAM::*m)(std::vector<Point2f>&, std::vector<Point2f>&, std::vector<int>&, int) = &visualSLAM::removeDuplicates;
    std::vector<int> (visualOdometry::*o)(std::vector<Point2f>&, std::vector<Point2f>&, std::vector<int>&, int) =
        &visualOdometry::removeDuplicates;
    (void)m; (void)o;
    return 0;
}
''')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", *extra, f"-I{ROOT / 'include'}", str(tu)],
                   check=True, capture_output=True, text=True)


def build_smoke(exe, extra=()):
    src = ROOT / "tests" / "cpp" / "replenish_smoke.cpp"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *extra, f"-I{ROOT / 'include'}", str(src),
                    f"-L{ROOT / 'ros_stereo_slam_amd'}", "-l:libsvo_hip.so", f"-Wl,-rpath,{ROOT / 'ros_stereo_slam_amd'}",
                    "-o", str(exe)], check=True, capture_output=True, text=True)


@pytest.mark.parametrize("extra", [(), tuple(REAL_TYPES)], ids=["pod", "opencv_eigen"])
def test_replenish_smoke_compiles_and_links(tmp_path, extra):
    build_smoke(tmp_path / "replenish_smoke", extra)


def test_default_radius_is_the_reference_s():
    for name in ("visualSLAM.hpp", "bundleAdjust.hpp"):
        text = (ROOT / "include" / "svo_compat" / name).read_text()
        assert "std::vector<int> &mask, int radius = 10)" in text and "remove_duplicates(ctx_," in text
    assert "SVO_DEDUP_DISC" in (ROOT / "include" / "svo_compat" / "types.hpp").read_text()


def test_host_arithmetic_under_the_sanitizers(tmp_path):
    """The refusals of both entry points, the capacity bound formed without overflow and the launch geometry up to 2^28 points, as a
    stand-alone program built with -fsanitize=address,undefined."""
    exe = tmp_path / "replenish_plan_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    str(ROOT / "tests" / "cpp" / "replenish_plan_check.cpp"), "-o", str(exe)], check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "replenish plan check ok" in out.stdout, (out.returncode, out.stdout, out.stderr)


def test_tile_constants_are_the_kernels():
    import replenish_fixtures as rf

    text = (ROOT / "ros_stereo_slam_amd" / "csrc" / "replenish_plan.hip.h").read_text()
    assert f"constexpr int BLOCK = {rf.BLOCK};" in text and f"constexpr int TILE = {rf.T};" in text
