"""The pose graph's host logic on its own, under the address and undefined-behaviour sanitizers: the elimination structure of a solve
(csrc/pg_solve_plan.hip.h: separators, segments, couplings, gather lists -- every index a kernel of posegraph.hip follows) and the
reader of .g2o files with the test of an information matrix (csrc/pg_g2o.hip.h), each through a stand-alone program of tests/cpp.
CPU only; tests/test_gpu_posegraph.py and tests/test_gpu_posegraph_info.py run the solves."""
import pathlib
import re
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
CSRC = ROOT / "ros_stereo_slam_amd" / "csrc"


def run_check(tmp_path, name, ok):
    exe = tmp_path / name
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    str(ROOT / "tests" / "cpp" / f"{name}.cpp"), "-o", str(exe)], check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and ok in out.stdout, (out.returncode, out.stdout, out.stderr)


def test_solve_plan_under_the_sanitizers(tmp_path):
    """Both ends, the cover and the cost model's choice on: two vertices; chains around the regular separator spacing (the tail
    segment of SEG_L rows); closures to the fixed vertex, between neighbours, with a shared endpoint, twice the same; ten closures
    between two segments (the surplus over PG_MAX_SEG_CHORDS promoted, the selection run again); the benchmark's 4541 vertices and
    40 closures; more separators than the separator solve's LDS holds (the refusal).  Every row in one segment or a separator, every
    source, term, Wc range and block of the gather lists inside what the kernels index with it."""
    run_check(tmp_path, "pg_solve_plan_check", "pg solve plan check ok")


def test_g2o_reader_under_the_sanitizers(tmp_path):
    """Round trips with and without the 21 information numbers, comments and unknown tags, vertex ids out of order, repeated, with
    a gap, negative; edges to a missing vertex and onto themselves; FIX 1; 20, 22 and 21-plus-junk information numbers, a non-finite
    entry, a non-positive pivot; no vertices, an empty file, no final newline, lines longer than the line buffer, a missing file:
    the parsed content or the exact text of the refusal."""
    run_check(tmp_path, "pg_g2o_check", "pg g2o check ok")


@pytest.mark.parametrize("header", ["pg_solve_plan.hip.h", "pg_g2o.hip.h"])
def test_the_headers_are_plain_host_code(header):
    text = (CSRC / header).read_text()
    assert "hip/hip_runtime" not in text and "__global__" not in text
    # (pg_g2o.hip.h marks pg_tri and q_normalize for the kernels too, through a macro that is empty without hipcc)
    assert "__device__" not in re.sub(r"#ifdef __HIPCC__.*?#endif", "", text, flags=re.S)
    assert f'#include "{header}"' in (CSRC / "posegraph.hip").read_text()
