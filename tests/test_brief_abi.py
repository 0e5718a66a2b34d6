"""svo_brief_* at the boundary: declared and exported, the Context methods present, the default test tables well formed, the
signatures of include/svo.h bound from C++ in both type builds of the compatibility headers, the adaptor's switch bound, the smoke
program compiled and linked (CPU only; tests/test_gpu_brief.py runs the program against the Python path)."""
import ctypes as C
import pathlib
import subprocess
import sys

import numpy as np
import pytest

from ros_stereo_slam_amd import capi

ROOT = pathlib.Path(__file__).resolve().parents[1]
REAL_TYPES = ["-DSVO_WITH_OPENCV", "-DSVO_WITH_EIGEN", f"-I{ROOT / 'tests' / 'cpp' / 'stubs'}"]
NAMES = ["svo_brief_default_pattern", "svo_brief_set_pattern", "svo_brief_describe_batch", "svo_brief_integral"]


def test_header_declares_and_library_exports():
    lib = capi.load()
    for name in NAMES:
        assert name in capi.declared_symbols()
        assert hasattr(lib, name)
    for m in ("brief_set_pattern", "brief_describe", "brief_integral"):
        assert hasattr(capi.Context, m)
    assert callable(capi.brief_default_pattern)
    assert (capi.K_BRIEF_INTEGRAL, capi.K_BRIEF_DESCRIBE) == (7, 8)


@pytest.mark.parametrize("nbytes", [16, 32, 64])
def test_default_pattern_is_a_gaussian_table(nbytes):
    pat = capi.brief_default_pattern(nbytes)
    assert pat.shape == (8 * nbytes, 4) and pat.dtype == np.int8
    assert np.abs(pat.astype(int)).max() <= 24
    assert not np.any((pat[:, 0] == pat[:, 2]) & (pat[:, 1] == pat[:, 3])), "a test with equal end points"
    assert len({tuple(r) for r in pat.tolist()}) == len(pat), "a duplicated test"
    ends = np.concatenate([pat[:, :2], pat[:, 2:]]).astype(np.float64)    # (y, x) of all end points
    for axis in (0, 1):
        assert abs(ends[:, axis].std() - 48 / 5) <= 1.5, f"axis {axis}: standard deviation {ends[:, axis].std():.2f}"
    assert np.array_equal(capi.brief_default_pattern(nbytes), pat)
    import brief_numpy as bn

    bn.check_table(pat, nbytes)


def test_default_pattern_refuses_other_lengths():
    lib = capi.load()
    buf = np.zeros(4096, np.int8)
    for bad in (0, 8, 24, 33, 128, -32):
        assert lib.svo_brief_default_pattern(bad, buf.ctypes.data_as(C.c_void_p)) == capi.SVO_ERR_ARG
        with pytest.raises(capi.SvoError) as e:
            capi.brief_default_pattern(bad)
        assert e.value.code == capi.SVO_ERR_ARG
    assert lib.svo_brief_default_pattern(32, None) == capi.SVO_ERR_ARG
    assert not buf.any()


def test_committed_tables_are_what_the_generator_draws():
    out = subprocess.run([sys.executable, str(ROOT / "tools" / "gen_brief_pattern.py")], check=True, capture_output=True, text=True).stdout
    assert out == (ROOT / "ros_stereo_slam_amd" / "csrc" / "brief_pattern.hip.h").read_text()


@pytest.mark.parametrize("extra", [(), tuple(REAL_TYPES)], ids=["pod", "opencv_eigen"])
def test_signatures_bind(tmp_path, extra):
    tu = tmp_path / "sig.cpp"
    tu.write_text('''
#include "svo_compat/stereoCV.hpp"
int main() {
    int (*d)(int, int8_t*) = &svo_brief_default_pattern;
    int (*s)(svo_ctx*, int, const int8_t*) = &svo_brief_set_pattern;
    int (*b)(svo_ctx*, const uint8_t* const*, int, int, int, int, int, const float*, const int*, int, int*, uint8_t*, int*, int) =
        &svo_brief_describe_batch;
    int (*i)(svo_ctx*, const uint8_t*, int, int, int, int32_t*, int) = &svo_brief_integral;
    (void)d; (void)s; (void)b; (void)i;
    using namespace svo_compat;
    bool StereoProcess::*flag = &StereoProcess::BRIEF_FLAG;
    int StereoProcess::*nf = &StereoProcess::siftFeaturesStereo;
    int StereoProcess::*nb = &StereoProcess::briefBytes;
    void (StereoProcess::*feat)(const Mat&, std::vector<KeyPoint>&, std::vector<uint8_t>&) = &StereoProcess::briefFeatures;
    void (StereoProcess::*tri)(const Mat&, const Mat&, std::vector<Point3f>&) = &StereoProcess::stereoTriangulate;  // include/stereoCV.h:62
    (void)flag; (void)nf; (void)nb; (void)feat; (void)tri;
    StereoProcess sp(nullptr);
    if (sp.BRIEF_FLAG || sp.SIFT_FLAG) return 2;   // off by default
    static_assert(SVO_K_BRIEF_INTEGRAL == 7 && SVO_K_BRIEF_DESCRIBE == 8 && SVO_K_COUNT == 9, "kernel ids");
    return sp.siftFeaturesStereo == 20000 && sp.briefBytes == 32 ? 0 : 1;
}
''')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", *extra, f"-I{ROOT / 'include'}", str(tu)],
                   check=True, capture_output=True, text=True)


def build_smoke(exe):
    src = ROOT / "tests" / "cpp" / "brief_stereo_smoke.cpp"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src),
                    f"-L{ROOT / 'ros_stereo_slam_amd'}", "-l:libsvo_hip.so", f"-Wl,-rpath,{ROOT / 'ros_stereo_slam_amd'}",
                    "-o", str(exe)], check=True, capture_output=True, text=True)


def test_brief_stereo_smoke_compiles_and_links(tmp_path):
    build_smoke(tmp_path / "brief_stereo_smoke")


def test_brief_stereo_smoke_compiles_against_the_stubs(tmp_path):
    src = ROOT / "tests" / "cpp" / "brief_stereo_smoke.cpp"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", *REAL_TYPES, f"-I{ROOT / 'include'}", str(src)],
                   check=True, capture_output=True, text=True)
