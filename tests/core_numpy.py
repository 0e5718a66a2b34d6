"""Plain numpy definitions of the per-frame operations: compaction, adaptive non-maximal suppression, colour lookup, the rigid
transform and DLT triangulation.  Written from what each operation is defined to compute (the reference call sites quoted in the
headers of csrc/anms.hip and csrc/geometry.hip), not from the kernels: no tiles, no waves, no prefix counts, float64 wherever
arithmetic is involved."""
import numpy as np


def compact(mask, *arrays):
    """The rows whose mask byte is exactly 1, in input order (src/tracking.cpp:20-27, 35-42, 66-84)."""
    keep = np.asarray(mask, np.uint8) == 1
    return [np.asarray(a)[keep] for a in arrays]


def anms_radii(xy, resp):
    """Sorted order (response descending, ties in input order) and each sorted point's squared suppression radius: the smallest
    squared distance (float32 differences, squared and summed in float64) to an earlier-sorted point whose response exceeds
    float32(1.11f * own); infinite when there is none (src/ANMS.cpp:18-50)."""
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    resp = np.asarray(resp, np.float32).reshape(-1)
    n = len(resp)
    order = np.array(sorted(range(n), key=lambda i: (-resp[i], i)), np.int64)
    r2 = np.full(n, np.inf)
    for s in range(1, n):
        i = order[s]
        thr = np.float32(resp[i] * np.float32(1.11))
        before = order[:s]
        dom = before[resp[before] > thr]
        if len(dom):
            d = (xy[i][None, :] - xy[dom]).astype(np.float64)      # the differences are float32, their squares are not
            r2[s] = np.min(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    return order, r2


def anms_select(order, r2, keep):
    """Every point whose radius reaches the ``keep``-th largest (0-based), in sorted order; all of them when n <= keep
    (src/ANMS.cpp:52-67; the reference reads out of bounds at n == keep)."""
    if len(order) <= keep:
        return order.astype(np.int32)
    dec = np.sort(r2)[::-1][keep]
    return order[r2 >= dec].astype(np.int32)


def anms(xy, resp, keep):
    return anms_select(*anms_radii(xy, resp), keep)


def get_colors(img, xy):
    """img[int(y), int(x)] as three floats: the cast truncates toward zero, the index is clamped into the image, a grey image
    gives its value three times (include/monoUtils.h:180-193)."""
    img = np.asarray(img)
    h, w, c = img.shape
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    x = np.clip(np.trunc(xy[:, 0].astype(np.float64)).astype(np.int64), 0, w - 1)
    y = np.clip(np.trunc(xy[:, 1].astype(np.float64)).astype(np.int64), 0, h - 1)
    px = img[y, x]
    px = px[:, :3] if c >= 3 else np.repeat(px[:, :1], 3, axis=1)
    return px.astype(np.float32)


def transform_points(Rt, xyz):
    """[R|t] (3 x 4, float64) applied to float32 points, rounded to float32 once (src/keyFrameManagement.cpp:20-30)."""
    Rt = np.asarray(Rt, np.float64).reshape(3, 4)
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3).astype(np.float64)
    return (xyz @ Rt[:, :3].T + Rt[:, 3]).astype(np.float32)


def triangulate(P1, P2, x1, x2):
    """cv::triangulatePoints by SVD (src/triangulation.cpp:142-160): per pair the right singular vector of the smallest singular
    value of the 4 x 4 DLT system, in float64.  -> (xyz [n, 3] float32 = the float32 vector dehomogenised, v [n, 4] float64 of unit
    length, sign free)."""
    P1, P2 = np.asarray(P1, np.float64), np.asarray(P2, np.float64)
    x1 = np.asarray(x1, np.float32).reshape(-1, 2)
    x2 = np.asarray(x2, np.float32).reshape(-1, 2)
    n = len(x1)
    xyz, v = np.zeros((n, 3), np.float32), np.zeros((n, 4))
    for i in range(n):
        A = np.array([x1[i, 0] * P1[2] - P1[0], x1[i, 1] * P1[2] - P1[1], x2[i, 0] * P2[2] - P2[0], x2[i, 1] * P2[2] - P2[1]],
                     np.float64)
        v[i] = np.linalg.svd(A)[2][-1]
        v32 = v[i].astype(np.float32)
        with np.errstate(divide="ignore", invalid="ignore"):
            xyz[i] = v32[:3] / v32[3]
    return xyz, v
