#!/usr/bin/env python3
"""Draws the default BRIEF test tables of ros_stereo_slam_amd/csrc/brief_pattern.hip.h.

OpenCV's generated_16.i / generated_32.i / generated_64.i are not part of this project, so the library ships tables of its own,
drawn the way the BRIEF paper's "G II" does (Calonder et al., ECCV 2010): both end points of a test isotropic Gaussian around
the key point with sigma = PATCH_SIZE / 5 = 48 / 5.  A coordinate is rounded to the nearest integer and clamped to +-24, a test
whose end points coincide or that the table already holds (in either order) is drawn again.  One seeded generator draws the
three tables one after the other: 128, 256 and 512 rows of (y1, x1, y2, x2).

    python tools/gen_brief_pattern.py > ros_stereo_slam_amd/csrc/brief_pattern.hip.h

The output is committed; the library never runs this script."""
import numpy as np

SEED = 0x42524945  # "BRIE"
SIGMA = 48 / 5
HALF = 24


def draw_table(rng, n_tests):
    rows, seen = [], set()
    while len(rows) < n_tests:
        y1, x1, y2, x2 = (int(v) for v in np.clip(np.rint(rng.normal(0.0, SIGMA, 4)), -HALF, HALF))
        if (y1, x1) == (y2, x2) or (y1, x1, y2, x2) in seen or (y2, x2, y1, x1) in seen:
            continue
        seen.add((y1, x1, y2, x2))
        rows.append((y1, x1, y2, x2))
    return rows


def main():
    rng = np.random.default_rng(SEED)
    print("// brief_pattern.hip.h -- the default BRIEF test tables: rows of (y1, x1, y2, x2), both end points Gaussian with sigma 48 / 5,")
    print("// clamped to +-24.  Written by tools/gen_brief_pattern.py (seed 0x%X); do not edit by hand." % SEED)
    print("#pragma once")
    print("#include <cstdint>")
    for nbytes in (16, 32, 64):
        rows = draw_table(rng, 8 * nbytes)
        print(f"\nstatic const int8_t BRIEF_DEFAULT_{nbytes}[{8 * nbytes} * 4] = {{")
        for k in range(0, len(rows), 6):
            print("    " + "  ".join(",".join(f"{v:3d}" for v in r) + "," for r in rows[k:k + 6]))
        print("};")


if __name__ == "__main__":
    main()
