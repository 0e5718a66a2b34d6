"""svo_ba_window at the boundary: declared and exported, the parameter block's size, offsets and defaults (header == ctypes), every
refusal that needs no device with its outputs untouched, the adaptor's member bound from C++ in both type builds of the compatibility
headers, the smoke program compiled and linked, and the host arithmetic of csrc/ba_window.hip (ba_window_plan.hip.h) run on its own
under the address and undefined-behaviour sanitizers (CPU only; tests/test_gpu_ba_window.py runs the kernels)."""
import ctypes as C
import pathlib
import subprocess

import numpy as np
import pytest

import ba_window_fixtures as F
from ros_stereo_slam_amd import capi

ROOT = pathlib.Path(__file__).resolve().parents[1]
REAL_TYPES = ["-DSVO_WITH_OPENCV", "-DSVO_WITH_EIGEN", f"-I{ROOT / 'tests' / 'cpp' / 'stubs'}"]
NAMES = ["svo_ba_window", "svo_ba_window_default_params"]


def load_library():
    """torch ships its own HIP runtime: let it load first, as the ctx fixture of tests/conftest.py does, so that one copy serves torch and
    libsvo_hip whichever test of a session comes first (this file sorts before every GPU test)."""
    import torch

    torch.cuda.is_available()
    return capi.load()


def test_header_declares_and_library_exports():
    lib = load_library()
    for name in NAMES:
        assert name in capi.declared_symbols()
        assert hasattr(lib, name)
    assert callable(capi.Context.ba_window) and issubclass(capi.ba_window_params, C.Structure)
    assert lib.svo_version() == 100
    from ros_stereo_slam_amd import local_ba

    for m in ("open", "add", "adjust", "arrays"):
        assert callable(getattr(local_ba.KeyframeWindow, m))


def test_params_layout_is_the_header_s(tmp_path):
    tu = tmp_path / "layout.c"
    fields = [n for n, _ in capi.ba_window_params._fields_]
    tu.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "svo.h"\nint main(void) {\n'
                  '    printf("%zu", sizeof(svo_ba_window_params));\n' +
                  "".join(f'    printf(" %zu", offsetof(svo_ba_window_params, {n}));\n' for n in fields) + "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(tu), "-o", str(exe)], check=True,
                   capture_output=True, text=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == C.sizeof(capi.ba_window_params)
    assert got[1:] == [getattr(capi.ba_window_params, n).offset for n in fields]
    text = (ROOT / "include" / "svo.h").read_text()
    block = text[text.index("typedef struct svo_ba_window_params {"):text.index("} svo_ba_window_params;")]
    assert [n for n in fields if n in block] == fields


def test_defaults():
    p = capi.ba_window_params.default()
    assert (p.fx, p.fy, p.cx, p.cy) == (718.856, 718.856, 607.1928, 185.2157) and p.bf == 718.856 * 0.54
    assert p.iterations == 10 and p.huber_mono == 0.0 and p.huber_stereo == 0.0
    assert capi.ba_window_params.default(iterations=3, huber_mono=2.0).iterations == 3
    with pytest.raises(TypeError):
        capi.ba_window_params.default(nope=1)
    load_library().svo_ba_window_default_params(None)   # a null block is ignored


def refusals():
    """name -> (mutation of the argument dict, a word of the reason).  The base problem is valid."""
    def set_(key, value):
        return lambda a: a.__setitem__(key, value)

    def edit(key, index, value):
        def f(a):
            a[key] = a[key].copy()
            a[key][index] = value
        return f

    def params(**kw):
        return lambda a: a.__setitem__("prm", capi.ba_window_params.default(**{**F_PRM, **kw}))

    def all_held(a):
        a["fixed"] = np.ones_like(a["fixed"])

    def free17(a):
        a["n_poses"] = 18
        a["poses"] = np.tile(a["poses"][:1], (18, 1))
        a["fixed"] = np.r_[np.uint8(1), np.zeros(17, np.uint8)]

    def twice(a):
        s = a["obs_start"]
        i = int(np.flatnonzero(np.diff(s) >= 2)[0])
        a["obs_pose"] = a["obs_pose"].copy()
        a["obs_pose"][s[i] + 1] = a["obs_pose"][s[i]]

    return {
        "n_poses_0": (set_("n_poses", 0), "n_poses"), "n_poses_33": (set_("n_poses", 33), "n_poses"),
        "free_17": (free17, "more than 16"), "no_free": (all_held, "no free pose"),
        "n_points_0": (set_("n_points", 0), "n_points"), "n_points_neg": (set_("n_points", -3), "n_points"),
        "obs_pose_high": (edit("obs_pose", 4, 3), "out of range"), "obs_pose_neg": (edit("obs_pose", 0, -1), "out of range"),
        "start_decreases": (edit("obs_start", 2, 0), "decrease"), "start_not_0": (edit("obs_start", 0, 1), "begin at 0"),
        "seen_twice": (twice, "twice"), "starved_pose": (None, "fewer than three"),
        "iterations_neg": (params(iterations=-1), "iterations"), "huber_neg": (params(huber_stereo=-0.5), "Huber"),
        "stereo_bf_0": (params(bf=0.0), "bf"), "stereo_bf_neg": (params(bf=-1.0), "bf"),
        "mem_2": (set_("mem", 2), "mem"), "mem_neg": (set_("mem", -1), "mem"),
        "null_poses": (set_("poses", None), "null"), "null_fixed": (set_("fixed", None), "null"),
        "null_params": (set_("prm", None), "null"), "null_points": (set_("pts3d", None), "null"),
    }


F_PRM = dict(fx=F.K4[0], fy=F.K4[1], cx=F.K4[2], cy=F.K4[3], bf=F.BF)
# three poses, pose 0 held, four points: free pose 2 has three observations, free pose 1 only two; the last point has none
STARVED = (np.array([0, 3, 6, 8, 8], np.int32), np.array([0, 1, 2, 0, 1, 2, 0, 2], np.int32),
           np.tile(np.array([[300, 200, np.nan]], np.float32), (8, 1)))


def base_args():
    w = F.window(n=12, n_poses=3, seed=1)
    return dict(prm=capi.ba_window_params.default(**F_PRM), n_poses=3, poses=w["poses"].copy(), fixed=w["fixed"], n_points=12,
                pts3d=w["pts3d"], obs_start=w["obs_start"], obs_pose=w["obs_pose"], obs_uvr=w["obs_uvr"], mem=capi.MEM_HOST)


def call(lib, ctx_handle, a, outs):
    p = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)
    return lib.svo_ba_window(ctx_handle, None if a["prm"] is None else C.byref(a["prm"]), a["n_poses"], p(a["poses"]), p(a["fixed"]),
                             a["n_points"], p(a["pts3d"]), p(a["obs_start"]), p(a["obs_pose"]), p(a["obs_uvr"]), p(outs[0]),
                             p(outs[1]), p(outs[2]), a["mem"])


def fresh_outputs(a):
    return [np.full((max(a["n_points"], 1) + 40, 3), 7.25), np.full(len(a["obs_pose"]) + 8, 7.25), np.full(6, 7.25)]


@pytest.mark.parametrize("name", list(refusals()))
def test_refusals_need_no_device_and_touch_nothing(name):
    lib = load_library()
    mutate, word = refusals()[name]
    a = base_args()
    if name == "starved_pose":
        a["obs_start"], a["obs_pose"], a["obs_uvr"] = STARVED
        a["n_points"], a["pts3d"] = 4, np.ascontiguousarray(a["pts3d"][:4])
    else:
        mutate(a)
    poses_before = None if a["poses"] is None else a["poses"].copy()
    outs = fresh_outputs(a)
    rc = call(lib, None, a, outs)
    msg = lib.svo_last_error().decode()
    assert rc == capi.SVO_ERR_ARG and "svo_ba_window" in msg and word in msg, (rc, msg)
    assert all((o == 7.25).all() for o in outs)
    assert poses_before is None or np.array_equal(a["poses"], poses_before)


def test_a_valid_call_without_a_context_is_refused_for_the_context_alone():
    lib = load_library()
    a = base_args()
    before, outs = a["poses"].copy(), fresh_outputs(a)
    rc = call(lib, None, a, outs)
    assert rc == capi.SVO_ERR_ARG and "ctx must not be null" in lib.svo_last_error().decode()
    assert all((o == 7.25).all() for o in outs) and np.array_equal(a["poses"], before)
    a["n_points"] = (1 << 20) + 1
    assert call(lib, None, a, outs) == capi.SVO_ERR_CAPACITY and "2^20" in lib.svo_last_error().decode()


@pytest.mark.parametrize("extra", [(), tuple(REAL_TYPES)], ids=["pod", "opencv_eigen"])
def test_signatures_bind(tmp_path, extra):
    tu = tmp_path / "sig.cpp"
    tu.write_text('''
#include "svo_compat/bundleAdjust.hpp"
int main() {
    int (*a)(svo_ctx*, const svo_ba_window_params*, int, double*, const uint8_t*, int, const float*, const int*, const int*,
             const float*, double*, double*, double*, int) = &svo_ba_window;
    void (*b)(svo_ba_window_params*) = &svo_ba_window_default_params;
    (void)a; (void)b;
    static_assert(SVO_K_COUNT == 9, "no kernel id was added");
    static_assert(SVO_VERSION == 100, "the version stays");
    using namespace svo_compat;
    void (visualOdometry::*m)(std::vector<Mat>&, std::vector<Mat>&, const std::vector<unsigned char>&, const std::vector<Point3f>&,
                              const std::vector<int>&, const std::vector<int>&, const std::vector<float>&, Mat&, double,
                              std::vector<double>*, std::vector<double>*) = &visualOdometry::BundleAdjustWindow;
    (void)m;
    return 0;
}
''')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", *extra, f"-I{ROOT / 'include'}", str(tu)],
                   check=True, capture_output=True, text=True)


def build_smoke(exe, extra=()):
    src = ROOT / "tests" / "cpp" / "ba_window_smoke.cpp"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *extra, f"-I{ROOT / 'include'}", str(src),
                    f"-L{ROOT / 'ros_stereo_slam_amd'}", "-l:libsvo_hip.so", f"-Wl,-rpath,{ROOT / 'ros_stereo_slam_amd'}",
                    "-o", str(exe)], check=True, capture_output=True, text=True)


@pytest.mark.parametrize("extra", [(), tuple(REAL_TYPES)], ids=["pod", "opencv_eigen"])
def test_smoke_compiles_and_links(tmp_path, extra):
    build_smoke(tmp_path / "ba_window_smoke", extra)


def test_host_arithmetic_under_the_sanitizers(tmp_path):
    """The refusals and the CSR validation, the numbering of the free poses, the slab geometry up to 2^20 points, the packed triangle
    and the LM rule, as a stand-alone program built with -fsanitize=address,undefined."""
    exe = tmp_path / "ba_window_plan_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    str(ROOT / "tests" / "cpp" / "ba_window_plan_check.cpp"), "-o", str(exe)], check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "ba window plan check ok" in out.stdout, (out.returncode, out.stdout, out.stderr)


def test_fixture_constants_are_the_kernels():
    text = (ROOT / "ros_stereo_slam_amd" / "csrc" / "ba_window_plan.hip.h").read_text()
    assert f"constexpr int CHUNK = {F.CHUNK};" in text and f"constexpr int BLOCK = {F.BLOCK};" in text
    assert F.CONST["MAX_POSES"] == 32 and F.CONST["MAX_FREE"] == 16
