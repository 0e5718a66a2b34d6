"""The address arithmetic of the grey roles of pyramid.hip's base launch (csrc/pyr_grey_plan.hip.h: aligned dword loads of the raw
BGR rows, channel 0 picked by byte selectors, the tail guards, the deal of the level-0 items over a grid sized for three channels),
run on its own as a stand-alone program under the address and undefined-behaviour sanitizers over buffers of exactly the image's
size (CPU only; tests/test_gpu_pyr_grey_staging.py runs the kernels)."""
import pathlib
import subprocess

import pytest

import pyr_fixtures as pf

ROOT = pathlib.Path(__file__).resolve().parents[1]
WIDTHS, HEIGHTS = (44, 45, 46, 47, 128, 129, 130, 131, 132, 133, 135), (44, 45, 49, 51)
CASES = [(w, h, o) for w in WIDTHS for h in HEIGHTS for o in range(4)] + [(w, h, o) for o in (0, 3) for w, h in ((260, 66), (516, 132))]


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = tmp_path_factory.mktemp("pyr_grey_plan") / "pyr_grey_plan_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    str(ROOT / "tests" / "cpp" / "pyr_grey_plan_check.cpp"), "-o", str(exe)], check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "pyr grey plan check ok" in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
    rows = [tuple(int(x) for x in line.split()[1:]) for line in out.stdout.splitlines() if line.startswith("case ")]
    return {r[:3]: r[3:] for r in rows}


def test_every_lane_of_both_roles_under_the_sanitizers(report):
    """The program ended clean: no load outside a buffer, every byte equal to the per-byte gather, every item handed out once."""
    assert sorted(report) == sorted(CASES)


def test_the_dword_paths_are_taken(report):
    """(items, level-0 items by the dword path, interior tiles of level 1, their staged dwords) per case."""
    for (w, h, o), (items, l0_dword, l1_tiles, l1_dword) in report.items():
        assert items == ((w + 2 * pf.PYR_PAD + 15) // 16) * (h + 2 * pf.PYR_PAD)
        assert 0 < l0_dword < items, (w, h, o)       # every case is at least 44 wide: a group of sixteen lies inside a row
        assert l1_dword == l1_tiles * pf.SH * pf.nd(1)
        if w >= pf.RAW_FIRST_W and h >= pf.RAW_FIRST_H:
            assert l1_tiles > 0, (w, h, o)
        else:
            assert l1_tiles == 0, (w, h, o)


def test_constants_are_the_kernels():
    plan = (ROOT / "ros_stereo_slam_amd" / "csrc" / "pyr_grey_plan.hip.h").read_text()
    assert f"constexpr int PAD = {pf.PYR_PAD};" in plan and f"constexpr int LANES = {pf.PB};" in plan
    assert f"constexpr int TILE_W = {pf.TW}, TILE_H = {pf.TH};" in plan
    kernel = (ROOT / "ros_stereo_slam_amd" / "csrc" / "pyramid.hip").read_text()
    assert '#include "pyr_grey_plan.hip.h"' in kernel and "pgp::l0_group(" in kernel and "pgp::l1_stage_item(" in kernel
    assert "pgp::l0_run(" in kernel and "pgp::l1_tile_interior(" in kernel
