"""Named clouds for the voxel-grid down-sample, each with a proof -- taken from the restatement's own record (voxel_numpy) --
that it reaches the branch it is named for.  tests/test_voxel_numpy.py runs the proofs; tests/test_gpu_voxel.py runs every fixture
through the kernels.  Everything is built from seeds; colours are the library's B, G, R floats."""
import numpy as np

import voxel_numpy as vn

RS_TILE = 4096      # csrc/cloud_index.hip.h: elements of one radix-sort tile
SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8193]


def colours(n, seed):
    return np.random.default_rng(1000 + seed).uniform(0, 255, (n, 3)).astype(np.float32)


def random_cloud(n, seed=0, bad_every=0):
    """n points in [-2, 2)^3 for a leaf of 0.5 (about 500 voxels once n is large); bad_every > 0: every such point gets a NaN or an
    infinity in one coordinate"""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-2, 2, (n, 3)).astype(np.float32)
    if bad_every:
        bad = np.arange(bad_every // 2, n, bad_every)
        xyz[bad, bad % 3] = np.array([np.nan, np.inf, -np.inf], np.float32)[(bad // 3) % 3]
    return xyz


def _f32(rows):
    return np.array(rows, np.float32).reshape(-1, 3)


def exact_integer():
    """min 0, leaf 0.5: min_bound -0.25; x = 0.75 has (p - min_bound) / v = 1.0 / 0.5 = 2 exactly -- on a cell's lower face"""
    return _f32([[0, 0, 0], [0.75, 0, 0], [0.74999994, 0, 0], [1.25, 0.75, 0.25]]), 0.5


def minimum_point():
    """the minimum of every axis sits at reference coordinate exactly 0.5 (leaf a power of two: the subtractions are exact)"""
    return _f32([[-3.5, 2.25, 7], [1, 2.25, 9], [-3.5, 4, 7.125], [0, 3, 8]]), 0.25


def negative():
    rng = np.random.default_rng(3)
    return (-rng.uniform(0.5, 40, (300, 3))).astype(np.float32), 1.5


def leaf_tenth():
    """leaf 0.1, which no double holds"""
    return random_cloud(500, 4), 0.1


def division_not_reciprocal():
    """found by search (leaf 0.1, minimum 0, x in float32 near the cell faces) and kept: x = 0.25 has p - min_bound = 0.3, and
    0.3 / 0.1 = 2.9999999999999996 -> cell 2 while 0.3 * (1 / 0.1) = 3.0000000000000004 -> cell 3.  x = 2.25 likewise (22 / 23)."""
    return _f32([[0, 0, 0], [0.25, 0, 0], [0.3, 0, 0], [2.25, 0, 0], [2.2, 0, 0]]), 0.1


def one_voxel():
    return np.random.default_rng(6).uniform(0, 0.4, (777, 3)).astype(np.float32), 1.0


def own_voxels():
    g = np.stack(np.meshgrid(np.arange(7), np.arange(6), np.arange(5), indexing="ij"), -1).reshape(-1, 3)
    return np.random.default_rng(7).permutation(g).astype(np.float32), 0.5


def duplicates():
    base = random_cloud(40, 8)
    return np.concatenate([base, base[::2], base, base[:5]]), 0.5


def float_sum_differs():
    """2^24, 1, 1 (and a second voxel of two points beside it): a float accumulator loses both ones, the double one does not"""
    return _f32([[16777216, 5, 5], [1, 5, 5], [1, 5, 5], [3e9, 5, 5], [3e9, 5, 6]]), 1e9


def order_dependent():
    """1e17, 1, -1e17 in one voxel at a leaf of 1e18: (1e17 + 1) + -1e17 = 0 in double, (1e17 + -1e17) + 1 = 1"""
    return _f32([[1e17, 0, 0], [1, 0, 0], [-1e17, 0, 0]]), 1e18


def nonfinite_ends():
    """NaN and +-inf at the first, a middle and the last index"""
    xyz = random_cloud(301, 11)
    xyz[0, 1] = np.nan
    xyz[150, 0] = np.inf
    xyz[151, 2] = -np.inf
    xyz[300] = [np.nan, np.inf, 1]
    return xyz, 0.5


def all_nonfinite():
    xyz = random_cloud(70, 12)
    xyz[np.arange(70), np.arange(70) % 3] = np.array([np.nan, np.inf, -np.inf], np.float32)[np.arange(70) % 3]
    return xyz, 0.5


def cells_edge(refused: bool, axis=0):
    """leaf 1, minimum 0: the largest coordinate 2097151 lies in cell 2^21 - 1, the axis spans 2^21 cells (refused); 2097150 is one
    cell fewer (accepted).  Floats hold both exactly."""
    xyz = _f32([[0, 0, 0], [1, 1, 1], [0, 0, 0]])
    xyz[2, axis] = 2097151 if refused else 2097150
    return xyz, 1.0


def straddles_tiles():
    """8193 points: 100 in the lowest voxel, 4097 in the next -- sorted positions 100 .. 4196, across the seam of two radix tiles
    at 4096 --, the rest spread over many; the input order is shuffled"""
    rng = np.random.default_rng(14)
    # the minimum is 0 and the leaf 1, so min_bound = -0.5: cell 0 is [-0.5, 0.5), cell 1 is [0.5, 1.5)
    a = rng.uniform(0.0, 0.45, (100, 3))                              # cell (0, 0, 0): the lowest key
    b = rng.uniform(0.0, 0.45, (4097, 3)) + [0.55, 0, 0]              # cell (1, 0, 0): the next key
    c = rng.uniform(0.0, 20, (8193 - 4197, 3)) + [0, 0, 0.55]         # z cell >= 1: every key above
    xyz = np.concatenate([a, b, c]).astype(np.float32)
    xyz[0] = 0
    return xyz[rng.permutation(len(xyz))], 1.0


FIXTURES = {
    "exact_integer": exact_integer, "minimum_point": minimum_point, "negative": negative, "leaf_tenth": leaf_tenth,
    "division_not_reciprocal": division_not_reciprocal, "one_voxel": one_voxel, "own_voxels": own_voxels, "duplicates": duplicates,
    "float_sum_differs": float_sum_differs, "order_dependent": order_dependent, "nonfinite_ends": nonfinite_ends,
    "all_nonfinite": all_nonfinite, "cells_edge_accepted": lambda: cells_edge(False), "straddles_tiles": straddles_tiles,
}


def build(name):
    """-> (xyz, colour, leaf) of a named fixture"""
    xyz, leaf = FIXTURES[name]()
    return xyz, colours(len(xyz), sorted(FIXTURES).index(name)), leaf


_cache = {}


def expected(name, with_colour=True):
    """the restatement's answer for a fixture, computed once and shared: (xyz_out, colour_out, point_voxel, voxel_count, record)"""
    key = (name, with_colour)
    if key not in _cache:
        xyz, col, leaf = build(name)
        rec = {}
        out = vn.voxel_downsample(xyz, leaf, col if with_colour else None, record=rec)
        for a in out:
            if a is not None:
                a.setflags(write=False)
        _cache[key] = out + (rec,)
    return _cache[key]
