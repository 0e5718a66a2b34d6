"""The disparity WLS filter's C ABI and C++ adaptor: declared, exported, the parameter struct and its defaults the same in
the header and in ctypes, and the smoke program of StereoProcess's WLS_FLAG compiled in both type builds and linked."""
import ctypes as C
import pathlib
import re
import subprocess

import pytest

from ros_stereo_slam_amd import capi

ROOT = pathlib.Path(__file__).resolve().parents[1]
REAL_TYPES = ["-DSVO_WITH_OPENCV", "-DSVO_WITH_EIGEN", f"-I{ROOT / 'tests' / 'cpp' / 'stubs'}"]
NEW = ["svo_wls_default_params", "svo_sgbm_right_matcher_params", "svo_wls_filter", "svo_sgbm_wls_compute"]
FIELDS = ["lambda", "sigma_color", "lrc_thresh", "depth_discontinuity_radius", "roll_off", "use_confidence", "roi_left",
          "roi_right", "roi_top", "roi_bottom"]


def test_header_declares_and_library_exports():
    names = capi.declared_symbols()
    assert all(n in names for n in NEW)
    lib = capi.load()
    assert all(hasattr(lib, n) for n in NEW)
    assert all(hasattr(capi.Context, n) for n in ("wls_filter", "sgbm_wls"))
    assert callable(capi.wls_params) and callable(capi.sgbm_right_params)


def test_struct_and_defaults_agree_between_header_and_ctypes(tmp_path):
    text = (ROOT / "include" / "svo.h").read_text()
    body = re.search(r"typedef struct svo_wls_params \{(.*?)\} svo_wls_params;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [(t, n.strip()) for t, names in re.findall(r"(double|int|float)\s+([^;]+);", body) for n in names.split(",")]
    ctype = {"double": C.c_double, "int": C.c_int, "float": C.c_float}
    assert [n for _, n in declared] == FIELDS
    assert [(ctype[t], n.rstrip("_")) for t, n in declared] == [(t, n.rstrip("_")) for n, t in capi.WlsParams._fields_]
    # the header as a C compiler lays it out, and the defaults as the library fills them
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "svo.h"\nint main(void) {\n'
                   '    svo_sgbm_params s; svo_wls_params p; svo_sgbm_default_params(&s); svo_wls_default_params(&s, &p);\n'
                   '    printf("%zu", sizeof(svo_wls_params));\n'
                   + "".join(f'    printf(" %zu", offsetof(svo_wls_params, {f}));\n' for f in FIELDS) +
                   '    printf("\\n%.17g %.17g %d %d %.17g %d %d %d %d %d\\n", p.lambda, p.sigma_color, p.lrc_thresh,\n'
                   '           p.depth_discontinuity_radius, (double)p.roll_off, p.use_confidence, p.roi_left, p.roi_right, p.roi_top,\n'
                   '           p.roi_bottom);\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), f"-L{ROOT / 'ros_stereo_slam_amd'}",
                    "-l:libsvo_hip.so", f"-Wl,-rpath,{ROOT / 'ros_stereo_slam_amd'}", "-o", str(exe)], check=True,
                   capture_output=True, text=True)
    layout, values = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    sizes = [int(v) for v in layout.split()]
    assert sizes[0] == C.sizeof(capi.WlsParams) == 48
    assert sizes[1:] == [getattr(capi.WlsParams, n).offset for n, _ in capi.WlsParams._fields_]
    p = capi.wls_params()
    got = [getattr(p, n) for n, _ in capi.WlsParams._fields_]
    assert [float(v) for v in values.split()] == [float(v) for v in got]
    assert got[:4] == [8000.0, 1.5, 24, 4] and got[5:] == [1, 100, 3, 3, 3] and got[4] == C.c_float(0.001).value


def test_right_matcher_params_of_the_references_matcher():
    r = capi.sgbm_right_params(capi.sgbm_params())
    assert [getattr(r, n) for n, _ in r._fields_] == [-96, 96, 7, 24, 96, 1000000, 60, 0, 0, 0, 0]
    q = capi.wls_params(capi.sgbm_params(min_disparity=-8, num_disparities=32, block_size=3))
    assert (q.roi_left, q.roi_right, q.roi_top, q.roi_bottom, q.depth_discontinuity_radius) == (25, 9, 1, 1, 2)


@pytest.mark.parametrize("extra", [(), tuple(REAL_TYPES)], ids=["pod", "opencv_eigen"])
def test_wls_smoke_compiles_in_both_type_builds_and_links(tmp_path, extra):
    src = ROOT / "tests" / "cpp" / "wls_smoke.cpp"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *extra, f"-I{ROOT / 'include'}", str(src),
                    f"-L{ROOT / 'ros_stereo_slam_amd'}", "-l:libsvo_hip.so", f"-Wl,-rpath,{ROOT / 'ros_stereo_slam_amd'}",
                    "-o", str(tmp_path / "wls_smoke")], check=True, capture_output=True, text=True)


@pytest.mark.parametrize("extra", [(), tuple(REAL_TYPES)], ids=["pod", "opencv_eigen"])
def test_adaptor_members(tmp_path, extra):
    tu = tmp_path / "members.cpp"
    tu.write_text('''
#include "svo_compat/stereoCV.hpp"
using namespace svo_compat;
int main() {
    bool StereoProcess::*a = &StereoProcess::WLS_FLAG;
    double StereoProcess::*b = &StereoProcess::lambda;
    double StereoProcess::*c = &StereoProcess::sigma;
    Mat StereoProcess::*d = &StereoProcess::confidenceMap;
    Mat (StereoProcess::*e)(int) = &StereoProcess::stereoMatch;
    (void)a; (void)b; (void)c; (void)d; (void)e;
    return 0;
}
''')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", *extra, f"-I{ROOT / 'include'}", str(tu)],
                   check=True, capture_output=True, text=True)
