"""Voxel-grid down-sampling restated in numpy: the written form of ``svo_voxel_downsample`` / ``svo_voxel_grid`` (DESIGN.md
section 10o).  Written from the definition alone, not from csrc/voxel.hip; tests/test_voxel_numpy.py holds it against a separate
brute-force dictionary loop, tests/test_gpu_voxel.py holds the kernels against it bit for bit.

Open3D's ``PointCloud::VoxelDownSample`` AS RECALLED (geometry/PointCloud.cpp; nothing of it was at hand):
  R1  voxel_size <= 0 is an error.
  R2  voxel_min_bound = GetMinBound() - voxel_size * 0.5 (and a max bound likewise, used only for the size check); all in double,
      Open3D's points being double.
  R3  "voxel_size is too small" when voxel_size * INT_MAX < the largest extent.
  R4  every point: ref_coord = (point - voxel_min_bound) / voxel_size -- a division, per component --, voxel_index =
      (int)floor(ref_coord); the point is added to the accumulator of that index in an unordered_map.
  R5  an accumulator adds point, colour and normal component-wise in double, in the order the points come (ascending input index),
      and counts; the output point is sum / double(count).
  R6  ``voxel_down_sample_and_trace`` also reports which input points fell into which output point.
Hence the minimum point of an axis sits at ref_coord exactly 0.5 (R2, R4), in cell 0.

Choices of ours where Open3D leaves one open or where this library differs:
  C1  Input points and colours are float32 (the library's clouds); each is promoted to double first, sums and the division are
      double, the result is rounded to float32 once, at the store.
  C2  A point with a NaN or infinite coordinate is dropped before step R2 and takes part in nothing (svo_sor_filter_large's rule);
      its point_voxel is -1.  Open3D would carry it into the bounds.
  C3  Output order: Open3D's is the iteration order of an unordered_map, i.e. unspecified.  Ours is ascending key, key =
      (i_z << 42) | (i_y << 21) | i_x.
  C4  The size check (R3) becomes: cells[a] = the cell of the largest coordinate of axis a + 1; an axis with cells >= 2^21 is refused
      (``Capacity``) before any key is formed, so every index fits its 21 bits with room to spare.
  C5  The trace is two arrays: point_voxel[n] (the output row of every input point) and voxel_count[n_out].
  C6  No normals (they are estimated after the down-sample, as the multiway-registration recipe does).
Not PCL's VoxelGrid, which differs in kind: float centroids and a leaf origin at multiples of the leaf."""
import numpy as np

MAX_CELLS = 1 << 21
MAX_POINTS = 1 << 22
CELLS_SATURATED = np.iinfo(np.int64).max


class Capacity(Exception):
    """what the library answers with SVO_ERR_CAPACITY"""


def leaf_ok(voxel_size) -> bool:
    v = float(voxel_size)
    return v > 0.0 and v < np.inf


def voxel_grid(min_xyz, max_xyz, voxel_size):
    """-> (min_bound [3] float64, cells [3] int64, fits).  fits is False when an axis spans 2^21 cells or more (C4)."""
    if not leaf_ok(voxel_size):
        raise ValueError("voxel_size must be positive and finite")
    lo = np.asarray(min_xyz, np.float32).reshape(3)
    hi = np.asarray(max_xyz, np.float32).reshape(3)
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (hi >= lo).all()):
        raise ValueError("the bounds must be finite, max not below min")
    v = np.float64(voxel_size)
    min_bound = lo.astype(np.float64) - v * np.float64(0.5)
    with np.errstate(over="ignore"):
        q = np.floor((hi.astype(np.float64) - min_bound) / v)
    cells = np.array([int(x) + 1 if x < 2.0 ** 62 else CELLS_SATURATED for x in q], np.int64)
    return min_bound, cells, bool((cells < MAX_CELLS).all())


def cell_indices(xyz, min_bound, voxel_size):
    """[n, 3] int64: floor((p - min_bound) / voxel_size), a double subtraction then a double division (R4)"""
    p = np.asarray(xyz, np.float32).reshape(-1, 3).astype(np.float64)
    return np.floor((p - np.asarray(min_bound, np.float64)) / np.float64(voxel_size)).astype(np.int64)


def pack_keys(idx):
    idx = np.asarray(idx, np.int64)
    return (idx[:, 2] << 42) | (idx[:, 1] << 21) | idx[:, 0]


def ordered_sums(values, row, n_rows, rank):
    """sums[r] = ((v_0 + v_1) + v_2) + ... over the values of row r in the order given (rank = position inside the row); float64.
    One numpy addition per rank over the rows that are that long: left to right, no pairwise tree."""
    sums = np.zeros((n_rows, values.shape[1]), np.float64)
    if len(values) == 0:
        return sums
    order = np.argsort(rank, kind="stable")
    rs, rw, vs = rank[order], row[order], values[order]
    cuts = np.flatnonzero(np.diff(rs)) + 1
    for a, b in zip(np.concatenate([[0], cuts]), np.concatenate([cuts, [len(rs)]])):
        sums[rw[a:b]] = sums[rw[a:b]] + vs[a:b]  # the rows of one rank are distinct
    return sums


def voxel_downsample(xyz, voxel_size, color=None, record=None):
    """-> (xyz_out [n_out, 3] float32, color_out or None, point_voxel [n] int32, voxel_count [n_out] int32).
    record (optional dict) receives the intermediate values the fixtures' proofs read: finite, min_bound, cells, idx, keys."""
    if not leaf_ok(voxel_size):
        raise ValueError("voxel_size must be positive and finite")
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    col = None if color is None else np.ascontiguousarray(color, np.float32).reshape(-1, 3)
    n = len(xyz)
    if n > MAX_POINTS:
        raise Capacity("at most 2^22 points")
    point_voxel = np.full(n, -1, np.int32)
    finite = np.isfinite(xyz).all(axis=1) if n else np.zeros(0, bool)
    if record is not None:
        record.update(finite=finite)
    src = np.flatnonzero(finite)                      # ascending input index
    if len(src) == 0:
        return np.zeros((0, 3), np.float32), (None if col is None else np.zeros((0, 3), np.float32)), point_voxel, np.zeros(0, np.int32)
    pts = xyz[src]
    min_bound, cells, fits = voxel_grid(pts.min(axis=0), pts.max(axis=0), voxel_size)
    if record is not None:
        record.update(min_bound=min_bound, cells=cells)
    if not fits:
        raise Capacity("voxel_size is too small: an axis of the cloud spans 2^21 cells or more")
    idx = cell_indices(pts, min_bound, voxel_size)
    keys = pack_keys(idx)
    uniq, row = np.unique(keys, return_inverse=True)  # ascending key
    row = row.reshape(-1)
    n_out = len(uniq)
    count = np.bincount(row, minlength=n_out)
    # position of every point inside its voxel, in ascending input index
    by_row = np.argsort(row, kind="stable")
    start = np.concatenate([[0], np.cumsum(count)[:-1]])
    rank = np.empty(len(src), np.int64)
    rank[by_row] = np.arange(len(src)) - start[row[by_row]]
    values = pts.astype(np.float64) if col is None else np.concatenate([pts, col[src]], axis=1).astype(np.float64)
    mean = (ordered_sums(values, row, n_out, rank) / count.astype(np.float64)[:, None]).astype(np.float32)
    point_voxel[src] = row.astype(np.int32)
    if record is not None:
        record.update(idx=idx, keys=keys, src=src, row=row)
    return (np.ascontiguousarray(mean[:, :3]), (None if col is None else np.ascontiguousarray(mean[:, 3:])), point_voxel,
            count.astype(np.int32))
