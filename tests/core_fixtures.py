"""The seam table of the per-frame kernels (compaction, ANMS, colours, transform, triangulation, F-RANSAC, PnP-RANSAC, BA, SOR) and
the seeded inputs both tests/test_core_numpy.py (CPU: the inputs are not vacuous) and tests/test_gpu_core_seams.py (GPU) run on.

Every size is named after the boundary it sits on, with the line of the kernel the boundary comes from; the constants are read from
the kernels' sources, so a kernel whose tile changes moves its seams here too.  No size is above 2 100."""
import collections
import functools
import pathlib
import re

import numpy as np
from scipy.spatial.transform import Rotation as Rot

from geom_fixtures import BASELINE, project, scene_points, two_view

CSRC = pathlib.Path(__file__).resolve().parents[1] / "ros_stereo_slam_amd" / "csrc"


def kernel_constant(source, name):
    """``constexpr int NAME = value;`` of csrc/<source>."""
    m = re.search(rf"constexpr int {name} = (\d+);", (CSRC / source).read_text())
    assert m, f"{source} no longer defines {name}"
    return int(m.group(1))


WAVE = 64                                                    # a gfx950 wavefront; every kernel below indexes lanes as t & 63
KPW_LONE = kernel_constant("anms.hip", "KPW_LONE")           # anms.hip:48, key points per wave of a lone problem
KPW_GROUP = kernel_constant("anms.hip", "KPW_GROUP")         # anms.hip:47, ... of several problems in one launch
GATHER_T = kernel_constant("anms.hip", "GATHER_T")           # anms.hip:231, threads of the gather's one workgroup
BA_T = kernel_constant("ba.hip", "BA_T")                     # ba.hip:28, threads of the one BA workgroup
F_PHASE_A = kernel_constant("fransac.hip", "PHASE_A")        # fransac.hip:29, iterations of the first hypothesis phase
PNP_PHASE_A = kernel_constant("pnp.hip", "PNP_PHASE_A")      # pnp.hip:798, the same for PnP
POINT_T = 256                                                # geometry.hip:184, 198, 408, 418: transform / colours workgroup
TRI_T = 64                                                   # geometry.hip:355: triangulation launches 64 threads a workgroup
SOR_T = 256                                                  # sor.hip:22, 31, 106, 110: SOR's workgroups (four waves, a point per wave)
COMPACT_SEGS = 16                                            # geometry.hip:456: a launch has 16 segments ...
assert (KPW_LONE, KPW_GROUP, GATHER_T, BA_T) == (2, 8, 256, 256), "the seam table below is written for these tiles"


def compact_seg(n):
    """geometry.hip:456: seg = ceil(ceil(n / 16) / 64) * 64, whole 64-element strips."""
    return max((((n + COMPACT_SEGS - 1) // COMPACT_SEGS + WAVE - 1) // WAVE) * WAVE, WAVE)


Seam = collections.namedtuple("Seam", "n probes source")


def _around(b, probes, source):
    return [Seam(b - 1, probes + ": below", source), Seam(b, probes + ": at", source), Seam(b + 1, probes + ": above", source)]


SEAMS = {
    "compact": [Seam(0, "empty: block 0 still writes the count", "geometry.hip:264"),
                Seam(1, "one lane", "geometry.hip:284"), Seam(2, "two lanes", "geometry.hip:284")]
    + _around(WAVE, "wave 64: one segment becomes two, the first prefix count", "geometry.hip:263-280")
    + _around(2 * WAVE, "wave 64: a prefix of two strips", "geometry.hip:270")
    + _around(COMPACT_SEGS * WAVE, "compaction segment 64 -> 128 at 1024", "geometry.hip:456")
    + _around(2 * COMPACT_SEGS * WAVE, "compaction segment 128 -> 192 at 2048", "geometry.hip:456"),
    "anms": [Seam(1, "KPW 2: the second key point of the only wave is clamped", "anms.hip:70,136,195"),
             Seam(2, "KPW 2: one full wave", "anms.hip:63"),
             Seam(3, "KPW 2: a full wave and a clamped one", "anms.hip:70,136,195")]
    + _around(WAVE, "wave 64: the rank kernel's own stripe, then a stripe after it", "anms.hip:77-107")
    + _around(2 * WAVE, "wave 64: stripes before, inside and after the own one (no multiple of KPW 8 either side)", "anms.hip:79-107")
    + _around(GATHER_T, "workgroup 256: the gather's per = ceil(n / 256) goes 1 -> 2", "anms.hip:245")
    + [Seam(2 * GATHER_T - 1, "workgroup 256: per = 2, the last thread one short", "anms.hip:245-246"),
       Seam(2 * GATHER_T + 1, "workgroup 256: per = 3, threads past the end idle", "anms.hip:245-246"),
       Seam(4 * GATHER_T + 1, "workgroup 256: per = 5, sixteen stripes and one key point", "anms.hip:96-107,245")],
    "points": [Seam(0, "empty: no launch", "geometry.hip:349,406"), Seam(1, "one thread", "geometry.hip:81,190")]
    + _around(TRI_T, "wave 64: the triangulation workgroup", "geometry.hip:355")
    + _around(POINT_T, "workgroup 256: the transform workgroup", "geometry.hip:408")
    + [Seam(4 * POINT_T + 1, "workgroup 256: five workgroups, one live thread in the last", "geometry.hip:408")],
    "colors": [Seam(1, "one thread", "geometry.hip:205")] + _around(POINT_T, "workgroup 256: the colour workgroup", "geometry.hip:418"),
    "fransac": [Seam(17, "the smallest counts of the RANSAC branch (15 pairs on), no multiple of four", "fransac.hip:547")]
    + _around(WAVE, "wave 64: the scoring pass", "fransac.hip:547") + [Seam(66, "wave 64: 4 k + 2", "fransac.hip:547"),
                                                                      Seam(67, "wave 64: 4 k + 3", "fransac.hip:547")]
    + _around(256, "workgroup 256: one step of the scoring pass", "fransac.hip:547")
    + [Seam(799, "below the smallest size of the older tests, 4 k + 3", "fransac.hip:547")],
    "pnp": [Seam(5, "the minimal sample is the whole set", "pnp.hip:30"), Seam(6, "one point beyond the sample", "pnp.hip:30"),
            Seam(7, "two beyond", "pnp.hip:30"), Seam(8, "three beyond", "pnp.hip:30")]
    + _around(WAVE, "wave 64: the scoring and refinement sums", "pnp.hip:924") + _around(256, "workgroup 256: RED_STRIDE 257", "pnp.hip:924"),
    "ba": [Seam(2, "two lanes", "ba.hip:166")] + _around(WAVE, "wave 64 of the fixed-order reduction", "ba.hip:166")
    + _around(BA_T, "workgroup 256: the strided loop's second trip", "ba.hip:166-189")
    + _around(2 * BA_T, "workgroup 256: the third trip", "ba.hip:166-189"),
}


def sizes(op):
    return [s.n for s in SEAMS[op]]


assert max(s.n for op in SEAMS.values() for s in op) <= 2100

# svo_sor_filter: (n, mean_k) around the 256-thread workgroups with the neighbour count below, at and above n - 1 (sor.hip:39)
SOR_CASES = [(n, k) for n in (SOR_T - 1, SOR_T, SOR_T + 1) for k in (8, n - 2, n - 1, n, 300)] + [(WAVE + 1, WAVE), (WAVE, WAVE - 1)]

# ---------------------------------------------------------------------------------------------------------------- compaction
ODD_BYTES = (0x00, 0x02, 0x03, 0x7F, 0x80, 0x81, 0xFE, 0xFF)      # where a carry trick that counts bytes equal to 1 goes wrong
MASK_KINDS = ("d0.1", "d0.9", "ones", "zeros", "first", "last", "odd")


def compact_mask(n, kind):
    rng = np.random.default_rng(7000 + n)
    if kind in ("d0.1", "d0.9"):
        return (rng.uniform(size=n) < float(kind[1:])).astype(np.uint8)
    if kind == "ones":
        return np.ones(n, np.uint8)
    mask = np.zeros(n, np.uint8)
    if kind == "first" and n:
        mask[0] = 1
    if kind == "last" and n:
        mask[-1] = 1
    if kind == "odd":
        # every third byte is one of the odd values, the bytes beside it are ones: over a few dwords each odd value has stood in
        # each of a dword's four byte lanes, above and below a 0x01
        mask = (rng.uniform(size=n) < 0.5).astype(np.uint8)
        for j, p in enumerate(range(1, n, 3)):
            mask[p] = ODD_BYTES[(j + j // len(ODD_BYTES)) % len(ODD_BYTES)]
            mask[p - 1] = 1
            if p + 1 < n:
                mask[p + 1] = 1
    return mask


def compact_arrays(n):
    rng = np.random.default_rng(7100 + n)
    return [rng.normal(size=(n, st)).astype(np.float32) for st in (2, 3, 2)]


# ---------------------------------------------------------------------------------------------------------------- ANMS
ANMS_KINDS = ("random_tied", "lattice", "equal", "mixed_sign")


def anms_keeps(n):
    return sorted({0, 1, n // 2, n - 1, n, n + 1} - {-1})


@functools.lru_cache(maxsize=None)
def anms_input(kind, n):
    rng = np.random.default_rng(7200 + n + 10000 * ANMS_KINDS.index(kind))
    xy = rng.uniform(0, 1241, (n, 2)).astype(np.float32)
    resp = rng.uniform(0, 1, n).astype(np.float32)
    if kind == "random_tied":
        resp[rng.integers(0, n, n // 5)] = resp[0]                  # a fifth of the responses tied
    elif kind == "lattice":                                          # equal spacings: equal radii, also at the decision rank
        cols = int(np.ceil(np.sqrt(n)))
        xy = np.stack([np.arange(n) % cols, np.arange(n) // cols], 1).astype(np.float32) * 8
    elif kind == "equal":                                            # nothing dominates anything
        resp[:] = np.float32(0.37)
    elif kind == "mixed_sign":                                       # 1.11 x a negative response lies BELOW it: ties dominate
        resp = rng.uniform(-1, 1, n).astype(np.float32)
        resp[rng.integers(0, n, n // 5)] = resp[0]
        resp[n // 2] = 10.0                                          # one point far above: the runner-up has it as only dominator
        if n > 8:
            resp[:n // 8] = -np.abs(resp[:n // 8])
    xy.setflags(write=False)
    resp.setflags(write=False)
    return xy, resp


# ---------------------------------------------------------------------------------------------------------------- colours
COLOR_IMAGES = ((131, 97, 1), (131, 97, 3), (160, 120, 1), (160, 120, 3))     # (w, h, c); 131 * c is no multiple of the 16-byte pitch


@functools.lru_cache(maxsize=None)
def color_image(w, h, c):
    img = np.random.default_rng(7300 + w + c).integers(0, 256, (h, w, c), dtype=np.uint8)
    img.setflags(write=False)
    return img


def color_edge_points(w, h):
    """Where the clamp and the truncation decide: all magnitudes below 2^31 (the cast is defined), no NaN."""
    xs = [-0.5, -1.0, -1e6, w - 0.01, float(w), w + 0.5, 1e6]
    ys = [-0.5, -1.0, -1e6, h - 0.01, float(h), h + 0.5, 1e6]
    pts = [(x, h / 2 + 0.25) for x in xs] + [(w / 2 + 0.75, y) for y in ys]
    pts += [(0.0, 0.0), (w - 1.0, 0.0), (0.0, h - 1.0), (w - 1.0, h - 1.0)]                    # the four corners
    pts += [(-0.5, -0.5), (w + 0.5, -1.0), (-1e6, h + 0.5), (1e6, 1e6), (-0.99, h - 0.01), (0.99, 0.99)]   # both axes off at once
    return np.array(pts, np.float32)


def color_points(w, h, n):
    """n points: random ones inside the image, the edge list at the END (so that at n = 257 it lies across the 256-thread seam)."""
    rng = np.random.default_rng(7400 + n + w)
    edge = color_edge_points(w, h)
    inside = rng.uniform([0, 0], [w - 0.01, h - 0.01], (max(n - len(edge), 0), 2)).astype(np.float32)
    return np.concatenate([inside, edge])[-n:] if n >= len(edge) else edge[:n]


# ---------------------------------------------------------------------------------------------------------------- transform / DLT
RT = np.c_[Rot.from_rotvec([0.2, -0.1, 0.3]).as_matrix(), [1.5, -0.2, 10.0]]


def transform_input(n):
    return np.random.default_rng(7500 + n).uniform(-50, 50, (n, 3)).astype(np.float32)


def tri_input(n):
    """Stereo pairs with half a pixel of noise (the rays do not meet), and at the first and the last index of every wave a pair of
    zero disparity (a point at infinity) or of negative disparity (behind the camera), alternating, so that both kinds stand at
    both ends of a wave.  -> (x1, x2, zero_idx, neg_idx)"""
    rng = np.random.default_rng(7600 + n)
    X = scene_points(n, 7600 + n)
    a = project(X).astype(np.float32)
    b = (project(X, np.eye(3), np.array([-BASELINE, 0, 0])) + rng.normal(0, 0.5, (n, 2))).astype(np.float32).reshape(n, 2)
    zero, neg = [], []
    for w0 in range(0, n, WAVE):
        first, last = w0, min(w0 + WAVE, n) - 1
        (zero if (w0 // WAVE) % 2 == 0 else neg).append(first)
        if last != first:
            (neg if (w0 // WAVE) % 2 == 0 else zero).append(last)
    b[zero] = a[zero]
    b[neg] = a[neg] + np.float32([10.0, 0.0])
    return a.reshape(n, 2), b, np.array(zero, np.int64), np.array(neg, np.int64)


# what tests/test_oracle_geometry.py::test_triangulate_known_answer_and_numpy_dlt allows the oracle against the float64 SVD DLT
TRI_RTOL, TRI_ATOL, TRI_DIRECTION = 2e-4, 1e-4, 1e-5


def check_dlt(xyz, h, ref_xyz, ref_v, zero_idx, what):
    """A triangulation against tests/core_numpy.py::triangulate: the dehomogenised points within the tolerance above, the homogeneous
    vectors in the same direction up to sign; pairs of zero disparity (w ~ 0) through the homogeneous vector only."""
    finite = np.setdiff1d(np.arange(len(xyz)), zero_idx)
    direction = np.abs(np.abs(np.einsum("ij,ij->i", h.astype(np.float64), ref_v)) - 1)
    assert len(xyz) == 0 or direction.max() < TRI_DIRECTION, (what, "direction", direction.max())
    bad = ~np.isclose(xyz[finite], ref_xyz[finite], rtol=TRI_RTOL, atol=TRI_ATOL)
    assert not bad.any(), (what, "points", finite[bad.any(axis=1)], xyz[finite][bad], ref_xyz[finite][bad])


def ulp_distance(a, b):
    """Distance of two float32 arrays in units of the last place (adjacent floats: 1; +0 and -0: 0)."""
    def ordered(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(ordered(a) - ordered(b))


# ---------------------------------------------------------------------------------------------------------------- RANSAC
# (n, threshold) -> (outliers, seed): fixed by tests/test_core_numpy.py, which holds every case to a non-trivial answer of the
# oracle.  An inlier share below 0.68 keeps the adaptive bound log(0.01) / log(1 - w^7) above the first phase's 64 iterations.
FRANSAC_THRESHOLDS = (1.0, 3.0)
_F_SHARE = {17: 0.24, 63: 0.25, 64: 0.25, 65: 0.25, 66: 0.25, 67: 0.25, 255: 0.45, 256: 0.25, 257: 0.25, 799: 0.45}


def fransac_case(n, thr):
    n_out = int(round(_F_SHARE[n] * n))
    seed = 100 + n + int(thr)
    x1, x2, gt, *_ = two_view(n=n, n_out=n_out, seed=seed, noise=0.15)
    return x1, x2, gt, seed


# n -> (outliers, reprojection bound, seed).  A hypothesis needs more than four inliers (pnp.hip / oracle/pnp.c: count > M - 1), so
# at n = 5 the only non-empty answer is everything; from n = 6 on every case has outliers that stay out.
_PNP = {5: (0, 1.0, 1), 6: (1, 1.0, 2), 7: (1, 1.0, 3), 8: (2, 1.0, 4), 63: (15, 1.0, 5), 64: (16, 1.0, 6), 65: (16, 1.0, 7),
        255: (150, 1.0, 8), 256: (64, 1.0, 9), 257: (110, 1.0, 10)}


def pnp_case(n):
    n_out, err, seed = _PNP[n]
    rng = np.random.default_rng(7700 + n)
    X = scene_points(n, 7700 + n)
    R, t = Rot.from_rotvec([0.02, -0.05, 0.01]).as_matrix(), np.array([0.1, -0.05, -0.8])
    x = project(X, R, t).astype(np.float32) + rng.normal(0, 0.15, (n, 2)).astype(np.float32)
    out = rng.choice(n, n_out, replace=False)
    x[out] += rng.uniform(10, 50, (n_out, 2)).astype(np.float32)
    return X.astype(np.float32), x, np.setdiff1d(np.arange(n), out), err, seed
