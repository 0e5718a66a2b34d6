"""A blind numpy restatement of the duplicate filter and of the replenishing step as DESIGN.md section 10k defines them, the second
party beside the HIP kernels (csrc/replenish.hip).

TEST INFRASTRUCTURE.  Written from what the two sources do -- the prototype's removeDuplicate and the tail of its trackSequence
(src/ROSslam.py:156-169, 262-271), the C++ removeDuplicates (include/monoUtils.h:195-213) -- and NOT from the kernels: one query
point at a time, the prototype's two-stage x / y selection in float64, the C++ loop over the listed reference points with float32
differences and a float64 norm, the append as a plain Python loop.

dedup_box(ref_xy, new_xy, radius, ref_idx=None)  -> keep [n_new] uint8
dedup_disc(ref_xy, new_xy, radius, ref_idx=None) -> keep [n_new] uint8
replenish(ref_xy, ref_xyz, new_xy, new_xyz, radius, mode, Rt) -> (xy, xyz, n_dup, n_behind)
"""
import numpy as np

BOX, DISC = 0, 1


def _listed(ref_xy, ref_idx):
    """The reference points that take part, as float32 rows: all of them, or the listed ones in the list's order (repeats stay,
    entries outside the array are passed over)."""
    ref = np.asarray(ref_xy, np.float32).reshape(-1, 2)
    if ref_idx is None:
        return ref
    rows = [ref[j] for j in np.asarray(ref_idx, np.int64).reshape(-1) if 0 <= j < len(ref)]
    return np.array(rows, np.float32).reshape(-1, 2)


def dedup_box(ref_xy, new_xy, radius, ref_idx=None):
    """The prototype: the query points are float64, a point with a reference point strictly inside its box is zeroed, and what
    comes back is "x != 0" -- so a query point whose own x is 0 goes too."""
    ref = _listed(ref_xy, ref_idx).astype(np.float64)     # float32 against a float64 limit compares in float64: made explicit
    query = np.asarray(new_xy, np.float32).reshape(-1, 2).astype(np.float64)      # pts1 = np.array(...).astype(float)
    radius = float(radius)
    for i in range(len(query)):
        q = query[i].copy()
        xlo, xhi = q[0] - radius, q[0] + radius
        ylo, yhi = q[1] - radius, q[1] + radius
        in_x = ref[(ref[:, 0] > xlo) & (ref[:, 0] < xhi)]
        if in_x.shape[0] != 0:
            in_xy = in_x[(in_x[:, 1] > ylo) & (in_x[:, 1] < yhi)]
            if in_xy.shape[0] != 0:
                query[i] = np.array([0, 0])
    return (query[:, 0] != 0).astype(np.uint8)


def dedup_disc(ref_xy, new_xy, radius, ref_idx=None):
    """The C++ side: for every new point the listed reference points in turn, norm(p1 - p2) < radius with Point2f differences and
    cv::norm's double accumulation."""
    ref = _listed(ref_xy, ref_idx)
    new = np.asarray(new_xy, np.float32).reshape(-1, 2)
    radius = float(radius)
    keep = np.zeros(len(new), np.uint8)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(len(new)):
            d = ref - new[i]                                                  # p1 - p2 for every listed p1: float32
            dx, dy = d[:, 0].astype(np.float64), d[:, 1].astype(np.float64)
            in_range = bool((np.sqrt(dx * dx + dy * dy) < radius).any())      # the loop breaks at the first one: any
            keep[i] = 0 if in_range else 1
    return keep


def dedup(ref_xy, new_xy, radius, mode, ref_idx=None):
    return (dedup_box if mode == BOX else dedup_disc)(ref_xy, new_xy, radius, ref_idx)


def move(Rt, p):
    """One float32 point through a 3 x 4 float64 [R|t]: double products in the order x, y, z, then t, one rounding to float32."""
    Rt = np.asarray(Rt, np.float64).reshape(3, 4)
    x, y, z = (np.float64(v) for v in p)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.array([np.float32(Rt[r, 0] * x + Rt[r, 1] * y + Rt[r, 2] * z + Rt[r, 3]) for r in range(3)], np.float32)


def replenish(ref_xy, ref_xyz, new_xy, new_xyz, radius, mode, Rt):
    """The top-up: drop the duplicates of what is held, move the rest, keep what lies in front (z of the float32 result > 0), append
    in input order."""
    xy = [row for row in np.asarray(ref_xy, np.float32).reshape(-1, 2)]
    xyz = [row for row in np.asarray(ref_xyz, np.float32).reshape(-1, 3)]
    new_xy = np.asarray(new_xy, np.float32).reshape(-1, 2)
    new_xyz = np.asarray(new_xyz, np.float32).reshape(-1, 3)
    keep = dedup(ref_xy, new_xy, radius, mode)
    n_dup = n_behind = 0
    for i in range(len(new_xy)):
        if not keep[i]:
            n_dup += 1
            continue
        m = move(Rt, new_xyz[i])
        if m[2] > 0:
            xy.append(new_xy[i])
            xyz.append(m)
        else:
            n_behind += 1
    return np.array(xy, np.float32).reshape(-1, 2), np.array(xyz, np.float32).reshape(-1, 3), n_dup, n_behind
