"""Seeded, small point sets for the duplicate filter and the replenishing step, each named for the branch it reaches;
tests/test_replenish_numpy.py proves from the restatement that it does.  A case is a dict: ref [n_ref, 2], new [n_new, 2] float32,
radius, mode, ref_idx (None or a list).  The largest holds 2 T + 1 reference points, T = 1024 the kernel's LDS tile."""
import numpy as np

BOX, DISC = 0, 1
T = 1024          # csrc/replenish_plan.hip.h: TILE
BLOCK = 256       # new points per workgroup
N_REF = (0, 1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1)
N_NEW = (0, 1, 63, 64, 65, 255, 256, 257)
FAR = 5000.0      # reference points parked here are near no new point


def case(ref, new, radius, mode, ref_idx=None):
    return dict(ref=np.asarray(ref, np.float32).reshape(-1, 2), new=np.asarray(new, np.float32).reshape(-1, 2), radius=float(radius),
                mode=mode, ref_idx=ref_idx)


def random_case(n_ref, n_new, mode, seed, radius=5.0, extent=None):
    """Points on a quarter-pixel lattice of a square sized so that a new point has about one reference point in its box: a good
    share of the new points has a neighbour, a good share has none, and offsets of exactly the radius occur."""
    rng = np.random.default_rng(seed)
    if extent is None:
        extent = max(20.0, 2.0 * radius * np.sqrt(max(n_ref, 1)))
    ref = rng.integers(0, int(extent * 4), (n_ref, 2)) / 4.0 + 1.0
    new = rng.integers(0, int(extent * 4), (n_new, 2)) / 4.0 + 1.0
    return case(ref, new, radius, mode)


def parked(n_ref, seed):
    """n_ref reference points far from the square the new points live in."""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 4000, (n_ref, 2)) / 4.0 + FAR).astype(np.float32)


def spread(n_new, seed, pitch=40.0):
    """New points far from one another (a lattice of pitch 40 with a little jitter), x never 0."""
    rng = np.random.default_rng(seed)
    k = np.arange(n_new)
    xy = np.stack([(k % 16) * pitch + 20.0, (k // 16) * pitch + 20.0], axis=1) + rng.integers(-8, 9, (n_new, 2)) / 4.0
    return xy.astype(np.float32)


def last_of_last_tile(mode):
    """2 T + 1 reference points: the only one near any new point is the LAST, alone in the third tile; it sits on new point 200."""
    ref, new = parked(2 * T + 1, 11), spread(257, 12)
    ref[-1] = new[200] + np.float32(1.0)
    return case(ref, new, 5.0, mode)


def early_exit(mode):
    """One workgroup of four waves.  Every lane of wave 0 (new points 0 ... 63) finds its neighbour in the FIRST tile (reference
    points 0 ... 63 sit on them); wave 3 (192 ... 255) has neighbours only in the LAST tile (reference point 2 T, near new point 250);
    waves 1 and 2 have none.  Wave 0 may skip the compares of tiles 1 and 2, and must still pass their barriers."""
    ref, new = parked(2 * T + 1, 21), spread(256, 22)
    ref[:64] = new[:64] + np.float32(0.5)
    ref[-1] = new[250] - np.float32(0.25)
    return case(ref, new, 5.0, mode)


def box_edge():
    """BOX, r = 5: |dx| == r exactly is outside (strict), the next float inwards is inside; the same on y and on the low side."""
    ref = [[100, 100]]
    inward = np.nextafter(np.float32(105), np.float32(0))
    new = [[105, 100], [inward, 100], [95, 100], [np.nextafter(np.float32(95), np.float32(200)), 100],
           [100, 105], [100, inward], [100, 95], [104, 104], [105, 105]]
    return case(ref, new, 5.0, BOX)


def box_corner(mode):
    """A point on the box's corner region: inside the box (|dx|, |dy| = 4.5 < 5), outside the disc (norm 6.36 > 5)."""
    return case([[100, 100]], [[104.5, 104.5], [103, 103], [95.5, 104.5]], 5.0, mode)


def disc_6_8():
    """DISC, r = 10: an offset of (6, 8) has norm exactly 10 and is no duplicate; the next float inwards on x is one; the
    same along the axes."""
    inward = np.nextafter(np.float32(106), np.float32(0))
    new = [[106, 108], [inward, 108], [94, 92], [100, 110], [100, np.nextafter(np.float32(110), np.float32(0))], [110, 100]]
    return case([[100, 100]], new, 10.0, DISC)


def disc_sqrt_ulp():
    """DISC with a radius that is no float: r = sqrt(s) rounded UP from an s the float differences reach, so that s < r * r and
    sqrt(s) < r may part.  dx = 3, dy = 1: s = 10, r = the double above sqrt(10) and the double below it."""
    r_exact = float(np.sqrt(np.float64(10.0)))
    return [case([[50, 50]], [[53, 51], [51, 53], [53.25, 51]], r, DISC)
            for r in (r_exact, float(np.nextafter(r_exact, 0.0)), float(np.nextafter(r_exact, 10.0)))]


def x_zero(mode):
    """The prototype's artefact: a new point whose own x is exactly 0 (also -0) goes in BOX mode though nothing is near it; y == 0
    does not matter.  In DISC mode all stay."""
    return case(parked(5, 31), [[0, 50], [-0.0, 70], [50, 0], [1e-30, 90], [30, 30]], 5.0, mode)


def nan_points(mode):
    """A NaN coordinate makes every comparison false: new points 0 ... 2 are kept although a reference point sits on their finite
    coordinate; the NaN reference points drop nobody; new point 3 has an honest neighbour."""
    nan = np.nan
    ref = [[5, 5], [nan, 20], [20, nan], [nan, nan], [40, 40]]
    new = [[nan, 5], [5, nan], [nan, nan], [41, 41], [20, 20]]
    return case(ref, new, 5.0, mode)


def listed(mode):
    """ref_idx: repeats, disorder, entries outside [0, n_ref) on both sides; the empty list; a list that names everything."""
    ref = [[10, 10], [50, 10], [90, 10], [130, 10], [170, 10]]
    new = [[11, 11], [51, 11], [91, 11], [131, 11], [171, 11], [300, 300]]
    lists = ([3, 1, 3, 3, 1], [4, -1, 5, 2, 1000000, -2147483648, 2147483647, 0], [], [0, 1, 2, 3, 4], [7, -3], [2])
    return [case(ref, new, 5.0, mode, ref_idx=list(l)) for l in lists]


def replenish_case(n_ref, n_new, mode, seed):
    """A held set, a fresh set with duplicates of it, 3-D points on both sides of the camera and an [R|t] that puts some survivors
    at z <= 0 and exactly one at z == 0: Rt's third row is (0, 0, 1, -2), so z' = z - 2, and the first survivor gets z = 2."""
    import replenish_numpy as rn

    c = random_case(n_ref, n_new, mode, seed)
    rng = np.random.default_rng(seed + 1000)
    ang = 0.1
    Rt = np.array([[np.cos(ang), 0, np.sin(ang), 0.25], [0, 1, 0, -0.125], [0, 0, 1, -2.0]])
    c["ref_xyz"] = rng.normal(0, 3, (n_ref, 3)).astype(np.float32)
    new_xyz = (rng.integers(-8, 40, (n_new, 3)) / 4.0).astype(np.float32)
    keep = rn.dedup(c["ref"], c["new"], c["radius"], mode)
    first = np.flatnonzero(keep)
    if len(first):
        new_xyz[first[0], 2] = 2.0
    c["new_xyz"], c["Rt"] = new_xyz, Rt
    return c
