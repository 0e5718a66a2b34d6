"""The numpy restatement of the voxel-grid down-sample (tests/voxel_numpy.py) against a brute-force dictionary loop written
separately, the proofs that every fixture of tests/voxel_fixtures.py reaches the branch it is named for, and the invariants of the
trace (CPU only; tests/test_gpu_voxel.py holds the kernels against the restatement)."""
import math

import numpy as np
import pytest

import voxel_fixtures as vf
import voxel_numpy as vn


def brute_force(xyz, leaf, color=None):
    """plain Python: a dictionary of cells, each a running double sum in input order"""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    good = [i for i in range(len(xyz)) if all(math.isfinite(float(c)) for c in xyz[i])]
    if not good:
        return [], [], [-1] * len(xyz), []
    mins = [min(float(xyz[i][a]) for i in good) for a in range(3)]
    mb = [mins[a] - leaf * 0.5 for a in range(3)]
    cells = {}
    for i in good:
        cell = tuple(math.floor((float(xyz[i][a]) - mb[a]) / leaf) for a in range(3))
        acc = cells.setdefault(cell, [[0.0] * 6, 0, []])
        vals = [float(v) for v in xyz[i]] + ([float(v) for v in color[i]] if color is not None else [0.0] * 3)
        acc[0] = [s + v for s, v in zip(acc[0], vals)]
        acc[1] += 1
        acc[2].append(i)
    order = sorted(cells, key=lambda c: (c[2], c[1], c[0]))
    pts, cols, pv, cnt = [], [], [-1] * len(xyz), []
    for row, cell in enumerate(order):
        s, k, members = cells[cell]
        pts.append([np.float32(v / float(k)) for v in s[:3]])
        cols.append([np.float32(v / float(k)) for v in s[3:]])
        cnt.append(k)
        for i in members:
            pv[i] = row
    return pts, cols, pv, cnt


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("name", sorted(vf.FIXTURES))
@pytest.mark.parametrize("with_colour", [False, True], ids=["xyz", "xyz_bgr"])
def test_restatement_equals_the_dictionary_loop(name, with_colour):
    xyz, col, leaf = vf.build(name)
    if len(xyz) > 2000:  # the Python loop is slow: the head of the big fixture, same leaf
        xyz, col = xyz[:2000], col[:2000]
        got = vn.voxel_downsample(xyz, leaf, col if with_colour else None)
    else:
        got = vf.expected(name, with_colour)[:4]
    pts, cols, pv, cnt = brute_force(xyz, leaf, col if with_colour else None)
    assert same_bits(got[0], np.array(pts, np.float32).reshape(-1, 3))
    if with_colour:
        assert same_bits(got[1], np.array(cols, np.float32).reshape(-1, 3))
    else:
        assert got[1] is None
    assert got[2].tolist() == pv and got[3].tolist() == cnt


@pytest.mark.parametrize("n", vf.SIZES)
def test_random_sizes_equal_the_dictionary_loop(n):
    xyz, col = vf.random_cloud(n, seed=n, bad_every=17 if n > 2 else 0), vf.colours(n, n)
    if n > 2000:
        xyz, col = xyz[-2000:], col[-2000:]
    got = vn.voxel_downsample(xyz, 0.5, col)
    pts, cols, pv, cnt = brute_force(xyz, 0.5, col)
    assert same_bits(got[0], np.array(pts, np.float32).reshape(-1, 3)) and same_bits(got[1], np.array(cols, np.float32).reshape(-1, 3))
    assert got[2].tolist() == pv and got[3].tolist() == cnt


@pytest.mark.parametrize("name", sorted(vf.FIXTURES))
def test_trace_invariants(name):
    xyz, _, leaf = vf.build(name)
    out, _, pv, cnt, rec = vf.expected(name)
    finite = np.isfinite(xyz).all(1)
    assert cnt.sum() == finite.sum() and len(out) == len(cnt) and (cnt > 0).all()
    assert ((pv >= 0) == finite).all() and (pv[~finite] == -1).all()
    assert np.array_equal(np.bincount(pv[finite], minlength=len(cnt)), cnt)
    if finite.any():
        assert (np.diff(np.unique(rec["keys"])) > 0).all() and rec["keys"].min() >= 0
        # rows ascend with the key: the row of a point is the rank of its key
        assert np.array_equal(np.unique(rec["keys"])[pv[finite]], rec["keys"])


@pytest.mark.parametrize("name", ["negative", "leaf_tenth", "own_voxels", "duplicates", "nonfinite_ends", "straddles_tiles"])
def test_rebinning_the_output_keeps_the_keys(name):
    """a voxel's mean lies inside the voxel, so binning the down-sampled cloud with the SAME min_bound gives every row its own key
    again -- away from a face: a mean may round onto it, which these fixtures do not do"""
    xyz, _, leaf = vf.build(name)
    out, _, _, _, rec = vf.expected(name)
    keys = vn.pack_keys(vn.cell_indices(out, rec["min_bound"], leaf))
    assert np.array_equal(keys, np.unique(rec["keys"]))


# ---- the proofs ---------------------------------------------------------------------------------------------------------------
def ref_coord(xyz, rec, leaf):
    return (np.asarray(xyz, np.float32).astype(np.float64) - rec["min_bound"]) / np.float64(leaf)


def test_proof_exact_integer():
    xyz, _, leaf = vf.build("exact_integer")
    rec = vf.expected("exact_integer")[4]
    r = ref_coord(xyz, rec, leaf)
    assert r[1, 0] == 2.0 and rec["idx"][1, 0] == 2          # on the face: the upper cell
    assert r[2, 0] < 2.0 and rec["idx"][2, 0] == 1           # one ulp of the float below: the lower cell
    assert vf.expected("exact_integer")[2][1] != vf.expected("exact_integer")[2][2]


def test_proof_minimum_point_sits_at_one_half():
    for name in ("minimum_point", "exact_integer", "division_not_reciprocal", "straddles_tiles"):
        xyz, _, leaf = vf.build(name)
        rec = vf.expected(name)[4]
        r = ref_coord(xyz, rec, leaf)
        for a in range(3):
            assert r[:, a].min() == 0.5 and rec["idx"][:, a].min() == 0


def test_proof_negative_and_leaf_tenth():
    xyz, _, leaf = vf.build("negative")
    assert (xyz < 0).all() and vf.expected("negative")[4]["idx"].min() == 0 and len(vf.expected("negative")[0]) > 50
    _, _, leaf = vf.build("leaf_tenth")
    assert leaf == 0.1 and np.float64(0.1).hex() == "0x1.999999999999ap-4"  # rounded up: not one tenth
    assert vf.expected("leaf_tenth")[4]["idx"].max() >= 39


def test_proof_division_not_reciprocal():
    xyz, _, leaf = vf.build("division_not_reciprocal")
    rec = vf.expected("division_not_reciprocal")[4]
    d = xyz.astype(np.float64) - rec["min_bound"]
    by_div, by_mul = np.floor(d / np.float64(leaf)), np.floor(d * (np.float64(1.0) / np.float64(leaf)))
    assert by_div[1, 0] == 2 and by_mul[1, 0] == 3 and by_div[3, 0] == 22 and by_mul[3, 0] == 23
    assert np.array_equal(rec["idx"], by_div.astype(np.int64))
    # with the reciprocal, 0.25 would share 0.3's cell; with the division it does not
    pv = vf.expected("division_not_reciprocal")[2]
    assert by_mul[1, 0] == by_mul[2, 0] and pv[1] != pv[2]


def test_proof_one_voxel_own_voxels_duplicates():
    out, _, pv, cnt, _ = vf.expected("one_voxel")
    assert len(out) == 1 and cnt.tolist() == [777] and (pv == 0).all()
    out, _, pv, cnt, _ = vf.expected("own_voxels")
    assert len(out) == 7 * 6 * 5 == len(pv) and (cnt == 1).all() and sorted(pv.tolist()) == list(range(210))
    xyz, _, _ = vf.build("own_voxels")
    assert same_bits(out[pv], xyz)   # the mean of one point is the point
    xyz, _, _ = vf.build("duplicates")
    out, _, pv, cnt, _ = vf.expected("duplicates")
    assert (pv[40:60] == pv[0:40:2]).all() and (pv[60:100] == pv[:40]).all() and cnt.max() >= 3


def test_proof_float_sum_differs():
    xyz, _, leaf = vf.build("float_sum_differs")
    out, _, pv, cnt, _ = vf.expected("float_sum_differs")
    assert pv.tolist() == [0, 0, 0, 1, 1] and cnt.tolist() == [3, 2]
    f = np.float32(0)
    for v in xyz[:3, 0]:
        f = np.float32(f + v)
    assert f == np.float32(16777216) and np.float32(f / np.float32(3)) != out[0, 0]
    assert out[0, 0] == np.float32(16777218.0 / 3.0)


def test_proof_order_dependent():
    xyz, col, leaf = vf.build("order_dependent")
    out = vf.expected("order_dependent")[0]
    assert len(out) == 1 and out[0, 0] == 0.0                      # (1e17 + 1) + -1e17: the one is lost
    perm = [0, 2, 1]
    other = vn.voxel_downsample(xyz[perm], leaf)[0]
    assert len(other) == 1 and other[0, 0] == np.float32(1.0 / 3.0)  # (1e17 + -1e17) + 1
    assert not same_bits(out, other)


def test_proof_nonfinite():
    xyz, _, _ = vf.build("nonfinite_ends")
    out, _, pv, cnt, rec = vf.expected("nonfinite_ends")
    assert pv[[0, 150, 151, 300]].tolist() == [-1] * 4 and (pv >= 0).sum() == 297 == cnt.sum()
    assert np.isfinite(out).all() and np.isfinite(rec["min_bound"]).all()
    out, col, pv, cnt, _ = vf.expected("all_nonfinite")
    assert out.shape == (0, 3) and col.shape == (0, 3) and (pv == -1).all() and len(pv) == 70 and len(cnt) == 0


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_proof_cells_edge(axis):
    xyz, leaf = vf.cells_edge(True, axis)
    mb, cells, fits = vn.voxel_grid(xyz.min(0), xyz.max(0), leaf)
    assert cells[axis] == 1 << 21 and not fits
    with pytest.raises(vn.Capacity):
        vn.voxel_downsample(xyz, leaf)
    xyz, leaf = vf.cells_edge(False, axis)
    mb, cells, fits = vn.voxel_grid(xyz.min(0), xyz.max(0), leaf)
    assert cells[axis] == (1 << 21) - 1 and fits
    rec = {}
    out, _, pv, cnt = vn.voxel_downsample(xyz, leaf, record=rec)
    assert rec["idx"][2, axis] == (1 << 21) - 2 and len(out) == 3 and sorted(pv.tolist()) == [0, 1, 2]
    assert int(rec["keys"][2]) == ((1 << 21) - 2) << (21 * axis)


def test_proof_straddles_tiles():
    xyz, _, _ = vf.build("straddles_tiles")
    out, _, pv, cnt, rec = vf.expected("straddles_tiles")
    assert len(xyz) == 8193 and cnt[0] == 100 and cnt[1] == 4097
    start, end = int(cnt[0]), int(cnt[0] + cnt[1])          # the sorted positions of the second voxel
    assert start < vf.RS_TILE < end and len(cnt) > 1000
    members = np.flatnonzero(pv == 1)
    assert len(members) == 4097 and (np.diff(members) > 0).all() and members[-1] - members[0] > 4097  # scattered over the input


def test_refusals_of_the_restatement():
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            vn.voxel_downsample(np.zeros((2, 3), np.float32), bad)
    out, col, pv, cnt = vn.voxel_downsample(np.zeros((0, 3), np.float32), 0.5, np.zeros((0, 3), np.float32))
    assert out.shape == (0, 3) and col.shape == (0, 3) and len(pv) == 0 and len(cnt) == 0
