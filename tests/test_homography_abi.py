"""The homography entry points at the boundary (CPU only; tests/test_gpu_homography.py runs the kernels): declared and
exported, the wrappers present, every refusal that needs no device with the outputs untouched, svo_decompose_homography
against the restatement, the adaptor's members in both type builds, the smoke program compiled and linked, and the host
code of the decomposition (homography_plan.hip.h) run on its own under the address and undefined-behaviour sanitizers."""
import ctypes as C
import pathlib
import subprocess

import numpy as np
import pytest

import homography_numpy as hn
from ros_stereo_slam_amd import capi
from test_homography_numpy import K4, decomposition_cases, rot

ROOT = pathlib.Path(__file__).resolve().parents[1]
REAL_TYPES = ["-DSVO_WITH_OPENCV", "-DSVO_WITH_EIGEN", f"-I{ROOT / 'tests' / 'cpp' / 'stubs'}"]
NAMES = ["svo_homography_4pt", "svo_find_homography", "svo_decompose_homography", "svo_homography_pose"]


def test_header_declares_and_library_exports():
    lib = capi.load()
    for name in NAMES:
        assert name in capi.declared_symbols() and hasattr(lib, name), name
    for m in ("homography_4pt", "find_homography", "homography_pose"):
        assert hasattr(capi.Context, m)
    assert callable(capi.decompose_homography)


def test_every_refusal_without_a_device_leaves_the_outputs_untouched():
    """decided before the context is looked at: a token stands in for it, nothing is launched"""
    lib = capi.load()
    token = C.c_void_p(C.addressof(C.create_string_buffer(64)))
    p = np.arange(40, dtype=np.float32).reshape(20, 2)

    def find(ctx=token, p1=p, p2=p, offsets=(0, 20), nprob=1, threshold=3.0, confidence=0.995, max_iters=2000, mem=capi.MEM_HOST,
             no_mask=False):
        mask, H, ints = np.full(20, 77, np.uint8), np.full(9, -77.0), np.full(2, -77, np.int32)
        off = np.ascontiguousarray(list(offsets) + [20] * 18, np.int32)
        rc = lib.svo_find_homography(ctx, capi._ptr(p1), capi._ptr(p2), capi._ptr(off), nprob, C.c_double(threshold),
                                     C.c_double(confidence), max_iters, C.c_uint64(1), None if no_mask else capi._ptr(mask),
                                     capi._ptr(H), capi._ptr(ints[:1]), capi._ptr(ints[1:]), mem)
        assert rc == capi.SVO_ERR_ARG and lib.svo_last_error()
        assert (mask == 77).all() and (H == -77).all() and (ints == -77).all()

    for kw in (dict(nprob=0), dict(nprob=17), dict(nprob=-1), dict(max_iters=0), dict(max_iters=20001), dict(p1=None), dict(p2=None),
               dict(no_mask=True), dict(offsets=(5, 3)), dict(offsets=(-1, 20)), dict(offsets=(0, 12, 8), nprob=2), dict(threshold=0.0),
               dict(threshold=float("nan")), dict(confidence=0.0), dict(confidence=1.0), dict(mem=2), dict(ctx=None)):
        find(**kw)

    def pose(ctx=token, H=np.eye(3).reshape(9), p1=p, p2=p, offsets=(0, 20), nprob=1, K=K4, dist=50.0, mem=capi.MEM_HOST):
        mask, R, t, n, g = np.full(20, 77, np.uint8), np.full(9, -77.0), np.full(3, -77.0), np.full(3, -77.0), np.full(4, -77, np.int32)
        off = np.ascontiguousarray(list(offsets) + [20] * 18, np.int32)
        Kh = None if K is None else np.ascontiguousarray(list(K) * 16, np.float64)
        rc = lib.svo_homography_pose(ctx, capi._ptr(H), capi._ptr(p1), capi._ptr(p2), capi._ptr(off), nprob, capi._ptr(Kh),
                                     C.c_double(dist), capi._ptr(mask), capi._ptr(R), capi._ptr(t), capi._ptr(n), capi._ptr(g), mem)
        assert rc == capi.SVO_ERR_ARG and lib.svo_last_error()
        assert (mask == 77).all() and (R == -77).all() and (t == -77).all() and (n == -77).all() and (g == -77).all()

    for kw in (dict(nprob=0), dict(nprob=17), dict(p1=None), dict(p2=None), dict(H=None), dict(offsets=(5, 3)), dict(K=None),
               dict(K=(0.0, 700.0, 1.0, 1.0)), dict(K=(700.0, float("inf"), 1.0, 1.0)), dict(dist=0.0), dict(mem=-1), dict(ctx=None)):
        pose(**kw)

    x = np.zeros((3, 4, 2))
    H, ok = np.full((3, 9), -77.0), np.full(3, -77, np.int32)
    for args in ((None, capi._ptr(x), capi._ptr(x), 3, capi._ptr(H), capi._ptr(ok), capi.MEM_HOST),
                 (token, capi._ptr(x), capi._ptr(x), -1, capi._ptr(H), capi._ptr(ok), capi.MEM_HOST),
                 (token, None, capi._ptr(x), 3, capi._ptr(H), capi._ptr(ok), capi.MEM_HOST),
                 (token, capi._ptr(x), capi._ptr(x), 3, None, capi._ptr(ok), capi.MEM_HOST),
                 (token, capi._ptr(x), capi._ptr(x), 3, capi._ptr(H), capi._ptr(ok), 7)):
        assert lib.svo_homography_4pt(*args) == capi.SVO_ERR_ARG
    assert (H == -77).all() and (ok == -77).all()
    assert lib.svo_homography_4pt(token, None, None, 0, None, None, capi.MEM_HOST) == capi.SVO_OK   # nothing to do

    for bad in (np.full(9, np.nan), np.r_[np.inf, np.zeros(8)]):
        with pytest.raises(capi.SvoError) as e:
            capi.decompose_homography(bad, K4)
        assert e.value.code == capi.SVO_ERR_ARG
    with pytest.raises(capi.SvoError):
        capi.decompose_homography(np.eye(3), (0.0, 1.0, 0.0, 0.0))


def test_decompose_homography_is_the_restatement():
    cases = decomposition_cases() + [(rot([0.03, -0.08, 0.02]), np.zeros(3), np.array([0, 0, 1.0]), 5.0)]
    rng = np.random.default_rng(5)
    for _ in range(100):
        n = rng.normal(size=3) * [0.4, 0.4, 0.1] + [0, 0, 1]
        cases.append((rot(rng.normal(size=3) * 0.1), rng.normal(size=3), n / np.linalg.norm(n), rng.uniform(2, 20)))
    counts = set()
    for R, t, n, d in cases:
        H = hn.homography_from_pose(R, t, n, d, K4) * rng.choice([-2.5, 1.0, 0.3])
        got, want = capi.decompose_homography(H, K4), hn.decompose(H, K4)
        assert len(got) == len(want)
        counts.add(len(got))
        for a, b in zip(got, want):
            for x, y in zip(a, b):
                assert np.array_equal(x, y)
    assert counts == {1, 4}
    assert capi.decompose_homography(np.zeros(9), K4) == [] and capi.decompose_homography(np.outer([1, 2, 3], [1, 1, 1.0]), K4) == []


@pytest.mark.parametrize("extra", [(), tuple(REAL_TYPES)], ids=["pod", "opencv_eigen"])
def test_adaptor_members(tmp_path, extra):
    tu = tmp_path / "sig.cpp"
    tu.write_text('''
#include "svo_compat/stereoCV.hpp"
using namespace svo_compat;
int main() {
    bool StereoProcess::*flag = &StereoProcess::HOMOGRAPHY_FLAG;
    double StereoProcess::*thr = &StereoProcess::homographyThreshold;
    double (StereoProcess::*nrm)[3] = &StereoProcess::planeNormal;
    void (StereoProcess::*m)(const Mat&, const Mat&, std::vector<Point3f>&) = &StereoProcess::monocularTriangulate;   // unchanged
    int (*a)(svo_ctx*, const double*, const double*, int, double*, int*, int) = &svo_homography_4pt;
    int (*b)(svo_ctx*, const float*, const float*, const int*, int, double, double, int, uint64_t, uint8_t*, double*, int*, int*, int) =
        &svo_find_homography;
    int (*c)(const double*, const double*, double*, double*, double*, int*) = &svo_decompose_homography;
    int (*d)(svo_ctx*, const double*, const float*, const float*, const int*, int, const double*, double, uint8_t*, double*, double*,
             double*, int*, int) = &svo_homography_pose;
    (void)flag; (void)thr; (void)nrm; (void)m; (void)a; (void)b; (void)c; (void)d;
    return 0;
}
''')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", *extra, f"-I{ROOT / 'include'}", str(tu)],
                   check=True, capture_output=True, text=True)


def test_the_flag_defaults_to_off():
    text = (ROOT / "include" / "svo_compat" / "stereoCV.hpp").read_text()
    assert "bool HOMOGRAPHY_FLAG = false;" in text and "double homographyThreshold = 3.0;" in text
    assert "if (HOMOGRAPHY_FLAG) {" in text


def build_smoke(exe, extra=()):
    src = ROOT / "tests" / "cpp" / "homography_mono_smoke.cpp"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *extra, f"-I{ROOT / 'include'}", str(src),
                    f"-L{ROOT / 'ros_stereo_slam_amd'}", "-l:libsvo_hip.so", f"-Wl,-rpath,{ROOT / 'ros_stereo_slam_amd'}",
                    "-o", str(exe)], check=True, capture_output=True, text=True)


@pytest.mark.parametrize("extra", [(), tuple(REAL_TYPES)], ids=["pod", "opencv_eigen"])
def test_smoke_compiles_and_links(tmp_path, extra):
    build_smoke(tmp_path / "homography_mono_smoke", extra)


def test_host_code_under_the_sanitizers(tmp_path):
    """homography_plan.hip.h as a stand-alone program with its own main, its host side built with
    -fsanitize=address,undefined and run directly"""
    exe = tmp_path / "homography_plan_check"
    subprocess.run(["hipcc", "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off",
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", f"-I{ROOT / 'include'}",
                    str(ROOT / "tests" / "cpp" / "homography_plan_check.cpp"), "-o", str(exe)], check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "homography plan check ok" in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
    rows = [[float(v) for v in line.split()[2:]] for line in out.stdout.splitlines() if line.startswith("sol ")]
    assert len(rows) == 4
    # the program's H, rebuilt here (products in another order: a few ulps apart), through the library
    cy, sy, cx, sx = np.cos(-0.05), np.sin(-0.05), np.cos(0.02), np.sin(0.02)
    R0 = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    n = np.array([0.5, 0.1, 1.0]) / np.linalg.norm([0.5, 0.1, 1.0])
    sols = capi.decompose_homography(hn.homography_from_pose(R0, np.array([0.6, -0.1, 0.4]) / 8, n, 1.0, K4), K4)
    for row, (R, t, nn) in zip(rows, sols):
        assert np.abs(np.r_[R.reshape(9), t, nn] - row).max() <= 1e-9
