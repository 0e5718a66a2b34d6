"""svo_match_cross, svo_radius_match and svo_knn_match_gated at the boundary: declared and exported, the struct's layout, the
wrappers present, every refusal decided without a device and with untouched outputs, the adaptors' members bound from C++ in both
type builds of the compatibility headers, the smoke program compiled and linked, and the host arithmetic of csrc/match.hip's new
calls (match_plan.hip.h) run on its own under the address and undefined-behaviour sanitizers (CPU only;
tests/test_gpu_match_ext.py runs the kernels)."""
import ctypes as C
import pathlib
import subprocess

import numpy as np
import pytest

import match_ext_numpy as mx
from ros_stereo_slam_amd import capi

ROOT = pathlib.Path(__file__).resolve().parents[1]
REAL_TYPES = ["-DSVO_WITH_OPENCV", "-DSVO_WITH_EIGEN", f"-I{ROOT / 'tests' / 'cpp' / 'stubs'}"]
NAMES = ["svo_match_cross", "svo_radius_match", "svo_knn_match_gated"]


def test_header_declares_and_library_exports():
    lib = capi.load()
    for name in NAMES + ["svo_knn_match", "svo_ratio_pairs"]:
        assert name in capi.declared_symbols() and hasattr(lib, name)
    for m in ("match_cross", "radius_match", "knn_match_gated", "knn_match", "ratio_pairs"):
        assert hasattr(capi.Context, m)
    assert (capi.CROSS_MUTUAL, capi.CROSS_CV) == (0, 1) == (mx.MUTUAL, mx.CV)
    assert capi.RADIUS_MAX_PER_QUERY == mx.MAX_PER_QUERY == 8192
    text = (ROOT / "include" / "svo.h").read_text()
    assert "enum { SVO_CROSS_MUTUAL = 0, SVO_CROSS_CV = 1 };" in text and "#define SVO_RADIUS_MAX_PER_QUERY 8192" in text
    assert C.sizeof(capi.MatchGate) == 12 and [f[0] for f in capi.MatchGate._fields_] == ["dy_max", "dx_min", "dx_max"]
    assert (capi.MatchGate.dy_max.offset, capi.MatchGate.dx_min.offset, capi.MatchGate.dx_max.offset) == (0, 4, 8)
    assert lib.svo_version() == 100


def test_struct_layout_and_signatures_bind(tmp_path):
    tu = tmp_path / "sig.c"
    tu.write_text('''
#include <stddef.h>
#include "svo.h"
_Static_assert(sizeof(svo_match_gate) == 12 && offsetof(svo_match_gate, dy_max) == 0 && offsetof(svo_match_gate, dx_min) == 4 &&
               offsetof(svo_match_gate, dx_max) == 8, "svo_match_gate");
_Static_assert(SVO_CROSS_MUTUAL == 0 && SVO_CROSS_CV == 1 && SVO_RADIUS_MAX_PER_QUERY == 8192, "constants");
int main(void) {
    int (*a)(svo_ctx*, int, const void*, const void*, int, const int*, const int*, int, int, int*, float*, int) = &svo_match_cross;
    int (*b)(svo_ctx*, int, const void*, const void*, int, const int*, const int*, int, float, int*, int*, float*, int, int*, int) = &svo_radius_match;
    int (*c)(svo_ctx*, int, const void*, const void*, int, const int*, const int*, int, int, const uint8_t*, const float*, const float*,
             const svo_match_gate*, int*, float*, int) = &svo_knn_match_gated;
    int (*k)(svo_ctx*, int, const void*, const void*, int, const int*, const int*, int, int, int*, float*, int) = &svo_knn_match;   /* unchanged */
    (void)a; (void)b; (void)c; (void)k;
    return 0;
}
''')
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", f"-I{ROOT / 'include'}", str(tu)],
                   check=True, capture_output=True, text=True)


class Args:
    """one problem of 4 x 5 rows of 32 floats with every output filled with a sentinel"""

    def __init__(self):
        self.q, self.t = np.zeros((4, 32), np.float32), np.zeros((5, 32), np.float32)
        self.qo, self.to = np.array([0, 4], np.int32), np.array([0, 5], np.int32)
        self.idx, self.dist = np.full(64, -7, np.int32), np.full(64, -8, np.float32)
        self.off, self.total = np.full(8, -9, np.int32), (C.c_int * 1)(-10)
        self.mask, self.xq, self.xt = np.ones((4, 5), np.uint8), np.zeros((4, 2), np.float32), np.zeros((5, 2), np.float32)
        self.gate = capi.MatchGate(1.0, 0.0, 2.0)

    def untouched(self):
        return (self.idx == -7).all() and (self.dist == -8).all() and (self.off == -9).all() and self.total[0] == -10


P = lambda a: None if a is None else (C.byref(a) if isinstance(a, C.Structure) else a.ctypes.data_as(C.c_void_p))


def call(lib, name, ctx, a, **o):
    v = dict(norm=0, q=a.q, t=a.t, dim=32, qo=a.qo, to=a.to, nprob=1, mem=capi.MEM_HOST, idx=a.idx, dist=a.dist, mode=0, r=1.0,
             off=a.off, cap=64, total=a.total, k=2, mask=None, xq=a.xq, xt=a.xt, gate=a.gate)
    v.update(o)
    head = (ctx, v["norm"], P(v["q"]), P(v["t"]), v["dim"], P(v["qo"]), P(v["to"]), v["nprob"])
    if name == "svo_match_cross":
        return lib.svo_match_cross(*head, v["mode"], P(v["idx"]), P(v["dist"]), v["mem"])
    if name == "svo_radius_match":
        tot = v["total"]
        return lib.svo_radius_match(*head, C.c_float(v["r"]), P(v["off"]), P(v["idx"]), P(v["dist"]), v["cap"],
                                    None if tot is None else tot, v["mem"])
    return lib.svo_knn_match_gated(*head, v["k"], P(v["mask"]), P(v["xq"]), P(v["xt"]), P(v["gate"]), P(v["idx"]), P(v["dist"]), v["mem"])


@pytest.mark.parametrize("name", NAMES)
def test_null_context_fails_cleanly_without_a_device(name):
    lib, a = capi.load(), Args()
    assert call(lib, name, None, a) == capi.SVO_ERR_ARG and lib.svo_last_error() and a.untouched()


@pytest.mark.parametrize("name", NAMES)
def test_every_refusal_leaves_the_outputs_untouched(name):
    """decided before the context is looked at: a token stands in for it, nothing is launched"""
    lib, a = capi.load(), Args()
    token = C.c_void_p(C.addressof(C.create_string_buffer(64)))

    def refused(code=capi.SVO_ERR_ARG, **over):
        assert call(lib, name, token, a, **over) == code and lib.svo_last_error(), over
        assert a.untouched(), over

    for norm in (-1, 3):
        refused(norm=norm)
    for norm, dim in ((0, 0), (0, 257), (1, 0), (1, 6), (1, 260), (2, 0), (2, 17)):
        refused(norm=norm, dim=dim)
    for nprob in (0, 17, -1):
        refused(nprob=nprob)
    for mem in (-1, 2):
        refused(mem=mem)
    refused(qo=None)
    refused(to=None)
    refused(qo=np.array([4, 0], np.int32))
    refused(to=np.array([5, 2], np.int32))
    refused(qo=np.array([-1, 3], np.int32))
    refused(q=None)
    refused(t=None)
    raw = np.zeros(5 * 32 * 4 + 4, np.uint8)
    off = raw[1:1 + 5 * 32 * 4].view(np.float32).reshape(5, 32)       # rows are read as 32-bit words
    refused(q=off[:4])
    refused(t=off)
    refused(idx=None)
    refused(dist=None)
    big = np.array([0, 32769], np.int32)                                # decided from the offsets alone: nothing is read
    refused(code=capi.SVO_ERR_CAPACITY, qo=big, dim=1)
    refused(code=capi.SVO_ERR_CAPACITY, to=big, dim=1)
    if name == "svo_match_cross":
        for mode in (-1, 2):
            refused(mode=mode)
    elif name == "svo_radius_match":
        refused(r=float("nan"))
        refused(cap=-1)
        refused(off=None)
        refused(total=None)
    else:
        for k in (0, 5):
            refused(k=k)
        refused(mask=a.mask)                                  # both forms
        refused(mask=None, gate=None)                         # neither
        refused(xq=None)
        refused(xt=None)
        refused(mask=a.mask, xq=None, xt=None)                # a mask and a gate


def test_wrappers_refuse_mixed_forms():
    with pytest.raises(AssertionError):
        capi.Context.knn_match_gated(None, np.zeros((1, 4), np.uint8), np.zeros((1, 4), np.uint8))
    with pytest.raises(AssertionError):
        capi.Context.knn_match_gated(None, np.zeros((1, 4), np.uint8), np.zeros((1, 4), np.uint8), mask=np.ones((1, 1)), gate=(1, 0, 1))


@pytest.mark.parametrize("extra", [(), tuple(REAL_TYPES)], ids=["pod", "opencv_eigen"])
def test_adaptor_members_bind(tmp_path, extra):
    tu = tmp_path / "sig.cpp"
    tu.write_text('''
#include "svo_compat/visualSLAM.hpp"
#include "svo_compat/stereoCV.hpp"
using namespace svo_compat;
using std::vector;
int main() {
    bool visualSLAM::*a = &visualSLAM::CROSS_CHECK_FLAG;
    bool visualSLAM::*b = &visualSLAM::EPIPOLAR_GATE_FLAG;
    float visualSLAM::*c = &visualSLAM::epipolarRows;
    float visualSLAM::*d = &visualSLAM::maxDisparity;
    bool StereoProcess::*e = &StereoProcess::CROSS_CHECK_FLAG;
    bool StereoProcess::*f = &StereoProcess::EPIPOLAR_GATE_FLAG;
    float StereoProcess::*g = &StereoProcess::epipolarRows;
    float StereoProcess::*h = &StereoProcess::maxDisparity;
    void (visualSLAM::*s)(const Mat&, const Mat&, vector<Point3f>&, vector<Point2f>&) = &visualSLAM::stereoTriangulate;  // unchanged
    (void)a; (void)b; (void)c; (void)d; (void)e; (void)f; (void)g; (void)h; (void)s;
    SparseMatch how;
    void (*m)(svo_ctx*, const SparseMatch&, int, const void*, const void*, int, int, int, const float*, const float*, vector<Point2f>&,
              vector<Point2f>&) = &sparse_match_points;
    (void)m;
    return how.cross || how.gate || how.epipolarRows != 2.0f;
}
''')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", *extra, f"-I{ROOT / 'include'}", str(tu)],
                   check=True, capture_output=True, text=True)


def test_the_flags_default_to_off():
    for header in ("visualSLAM.hpp", "stereoCV.hpp"):
        text = (ROOT / "include" / "svo_compat" / header).read_text()
        assert "bool CROSS_CHECK_FLAG = false;" in text and "bool EPIPOLAR_GATE_FLAG = false;" in text
        assert "float epipolarRows = 2.0f;" in text
    types = (ROOT / "include" / "svo_compat" / "types.hpp").read_text()
    assert "if (!how.cross && !how.gate) {\n        ratio_match_points(" in types     # both off: the reference's block


def build_smoke(exe, extra=()):
    src = ROOT / "tests" / "cpp" / "match_ext_smoke.cpp"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *extra, f"-I{ROOT / 'include'}", str(src),
                    f"-L{ROOT / 'ros_stereo_slam_amd'}", "-l:libsvo_hip.so", f"-Wl,-rpath,{ROOT / 'ros_stereo_slam_amd'}",
                    "-o", str(exe)], check=True, capture_output=True, text=True)


@pytest.mark.parametrize("extra", [(), tuple(REAL_TYPES)], ids=["pod", "opencv_eigen"])
def test_smoke_compiles_and_links(tmp_path, extra):
    build_smoke(tmp_path / "match_ext_smoke", extra)


def test_host_arithmetic_under_the_sanitizers(tmp_path):
    """The row words, the offset checks, the split (every tile owned once), the radius as a largest key on both sides of the
    answer and where neighbouring integer keys share a rooted float, the mask offsets beyond 32 bits, the CSR verdict and the
    sort's width, as a stand-alone program built with -fsanitize=address,undefined."""
    exe = tmp_path / "match_plan_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    str(ROOT / "tests" / "cpp" / "match_plan_check.cpp"), "-o", str(exe)], check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "match plan check ok" in out.stdout, (out.returncode, out.stdout, out.stderr)


def test_the_plan_header_is_plain_host_code_and_the_kernels_use_it():
    plan = (ROOT / "ros_stereo_slam_amd" / "csrc" / "match_plan.hip.h").read_text()
    assert "hip_runtime" not in plan and "__global__" not in plan
    assert "constexpr int MT = 32;" in plan and "constexpr int MQ = 256;" in plan and "constexpr int MAX_ROWS = 32768;" in plan
    match = (ROOT / "ros_stereo_slam_amd" / "csrc" / "match.hip").read_text()
    assert '#include "match_plan.hip.h"' in match
    for used in ("match_plan::plan(", "match_plan::radius_key_max(", "match_plan::mask_offsets(", "match_plan::csr_fits(",
                 "match_plan::sort_width(", "match_plan::sort_lds(", "match_plan::check_offsets(", "match_plan::words("):
        assert used in match, used
