"""A numpy / scipy restatement of svo_sor_filter_large (include/svo.h): the non-finite and z pre-filter, the mean
distance to the kk = min(mean_k, m - 1) nearest OTHER points with the float steps of the C code, the cloud statistics
summed in point order, keep d <= mean + mul * stddev.  Candidates come from a kd-tree; rows whose candidate list
cannot be proven to hold the kk smallest float squared distances (heavy duplication, near ties at its edge) are
redone by chunked brute force."""
import numpy as np
from scipy.spatial import cKDTree

EXTRA = 16          # candidates beyond kk + 1 asked of the kd-tree
ROWS = 20000        # queries per kd-tree batch
BRUTE_ROWS = 256    # queries per brute-force batch


def prefilter(xyz, z_limit):
    """Points that take part: every coordinate finite, and -z <= z_limit when z_limit > 0."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    keep = np.isfinite(xyz).all(axis=1)
    if z_limit > 0:
        with np.errstate(invalid="ignore"):
            keep &= ~(np.float32(-1.0) * xyz[:, 2] > np.float32(z_limit))
    return keep


def _sq_dist(q, o):
    """float32 (q - o)^2 summed x, y, z left to right, no fused multiply-add (q: [r, 1, 3], o: [r, c, 3])."""
    d = q - o
    d = d * d
    return (d[..., 0] + d[..., 1]) + d[..., 2]


def _mean_of_smallest(d2, kk):
    """float32 mean of sqrt of the kk smallest of every row: sqrt in float, summed ascending in float64."""
    s = np.sort(d2, axis=1)[:, :kk]
    r = np.sqrt(s).astype(np.float64)
    return (np.cumsum(r, axis=1)[:, -1] / kk).astype(np.float32)


def _brute_rows(p, rows, kk):
    out = np.empty(len(rows), np.float32)
    for s in range(0, len(rows), BRUTE_ROWS):
        r = rows[s:s + BRUTE_ROWS]
        d2 = _sq_dist(p[r][:, None, :], p[None, :, :])
        d2[np.arange(len(r)), r] = np.inf               # the query itself
        part = np.partition(d2, kk - 1, axis=1)[:, :kk]
        out[s:s + len(r)] = _mean_of_smallest(part, kk)
    return out


def mean_distances(p, mean_k):
    """float32 mean neighbour distance of every point of p (m x 3 float32, all finite)."""
    p = np.ascontiguousarray(p, np.float32)
    m = len(p)
    kk = min(mean_k, m - 1)
    if kk <= 0:
        return np.zeros(m, np.float32)
    k = min(m, kk + 1 + EXTRA)
    tree = cKDTree(p.astype(np.float64))
    out = np.empty(m, np.float32)
    redo = []
    for s in range(0, m, ROWS):
        q = np.arange(s, min(m, s + ROWS))
        dd, ii = tree.query(p[q].astype(np.float64), k=k, workers=-1)
        ii = ii.reshape(len(q), k)
        d2 = _sq_dist(p[q][:, None, :], p[ii])
        d2[ii == q[:, None]] = np.inf                   # drop the query's own index wherever it came
        part = np.sort(d2, axis=1)
        res = _mean_of_smallest(part, kk)
        if k < m:
            # proven only when the kk-th float value lies clearly below what any point outside the list can have
            far = dd.reshape(len(q), k)[:, -1] ** 2
            bad = ~(part[:, kk - 1].astype(np.float64) < far * (1 - 1e-5))
            redo.append(q[bad])
        out[q] = res
    if redo:
        rows = np.concatenate(redo)
        if len(rows):
            out[rows] = _brute_rows(p, rows, kk)
    return out


def threshold(dist, mul):
    """mean + mul * stddev with the sums in point order (sequential float64, the square in float32)."""
    m = len(dist)
    if m <= 1:
        return np.finfo(np.float64).max
    s = float(np.cumsum(dist.astype(np.float64))[-1])
    sq = float(np.cumsum((dist * dist).astype(np.float64))[-1])
    mean = s / m
    var = (sq - s * s / m) / (m - 1)
    if var < 0:
        var = 0.0
    return mean + mul * np.sqrt(var)


def sor_filter(xyz, color=None, mean_k=20, stddev_mul=0.8, z_limit=0.0):
    """-> (xyz_kept, color_kept or None, mean_dist), as Context.sor_filter_large returns them."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    keep0 = prefilter(xyz, z_limit)
    p = xyz[keep0]
    dist = mean_distances(p, mean_k)
    keep = dist.astype(np.float64) <= threshold(dist, stddev_mul)
    col = None
    if color is not None:
        col = np.asarray(color, np.float32).reshape(-1, 3)[keep0][keep]
    return p[keep], col, dist
