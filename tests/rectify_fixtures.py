"""Calibrations, maps and sources for the rectification tests (tests/test_rectify_numpy.py, test_rectify_abi.py,
test_gpu_rectify.py).  Everything is generated from constants and seeds."""
import functools

import numpy as np
from scipy.spatial.transform import Rotation as Rot

import rectify_numpy as rn


def _K(fx, fy, cx, cy):
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])


# name -> K1, D1, K2, D2, size, R, T
RIGS = {
    # EuRoC-like: 752 x 480, focal lengths near 458, k1 = -0.28, a rotation of about one degree, a baseline of 0.11 m
    "euroc": (_K(458.654, 457.296, 367.215, 248.375), [-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05],
              _K(457.587, 456.134, 379.999, 255.238), [-0.28368365, 0.07451284, -0.00010473, -3.55590700e-05], (752, 480),
              Rot.from_rotvec([0.003, -0.017, 0.002]).as_matrix(), np.array([-0.110, 0.0004, -0.0009])),
    # a vertical rig: the baseline lies along y, idx = 1
    "vertical": (_K(420.0, 421.5, 318.0, 242.0), [-0.11, 0.02, 0.0003, -0.0002, 0.001],
                 _K(419.0, 420.0, 322.5, 238.0), [-0.10, 0.015, -0.0001, 0.0004, 0.0], (640, 480),
                 Rot.from_rotvec([-0.012, 0.004, 0.006]).as_matrix(), np.array([0.002, -0.15, 0.001])),
    # the 8-coefficient rational model
    "rational": (_K(380.0, 381.0, 330.0, 235.0), [0.12, -0.03, 0.0004, -0.0003, 0.004, 0.25, -0.01, 0.002],
                 _K(382.0, 382.5, 318.0, 244.0), [0.11, -0.025, -0.0002, 0.0005, 0.005, 0.24, -0.008, 0.0015], (640, 480),
                 Rot.from_rotvec([0.008, 0.011, -0.004]).as_matrix(), np.array([-0.2, 0.003, 0.002])),
    # the reference's own case: one K, no distortion, no rotation (svo_stereo_rectify_q's)
    "identity": (_K(718.856, 718.856, 607.1928, 185.2157), None, _K(718.856, 718.856, 607.1928, 185.2157), None, (1241, 376),
                 np.eye(3), np.array([-0.54, 0.0, 0.0])),
}
WIDTHS = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257]  # around the quad, the wavefront's 64 quads... and a workgroup's 256 pixels
HEIGHTS = [1, 2, 3]


@functools.lru_cache(maxsize=None)
def rectification(name):
    K1, D1, K2, D2, size, R, T = RIGS[name]
    return rn.stereo_rectify(K1, D1, K2, D2, size, R, T)


@functools.lru_cache(maxsize=None)
def rig_maps(name):
    """-> ((xy, frac) of the left camera, (xy, frac) of the right one) at the rig's size"""
    K1, D1, K2, D2, size, _, _ = RIGS[name]
    R1, R2, P1, P2, _ = rectification(name)
    return rn.init_undistort_rectify_map(K1, D1, R1, P1, size), rn.init_undistort_rectify_map(K2, D2, R2, P2, size)


def tiny_camera(w, h):
    """a strongly distorted camera scaled to a tiny image, so that a few pixels span inside, border and far outside"""
    s = max(w, h, 4)
    return _K(0.9 * s, 0.8 * s, 0.45 * w, 0.55 * h), [-0.4, 0.15, 0.01, -0.02, 0.03], \
        Rot.from_rotvec([0.05, -0.04, 0.1]).as_matrix(), np.array([[0.7 * s, 0, 0.5 * w, 0], [0, 0.7 * s, 0.5 * h, 0], [0, 0, 1.0, 0]])


def source(sw, sh, c, seed):
    r = np.random.default_rng(seed).integers(0, 256, (sh, sw, c), dtype=np.uint8)
    return r if c == 3 else r[..., 0]


def words(x, y, fx=0, fy=0):
    """maps from integer tap arrays and fraction arrays"""
    x, y = np.asarray(x), np.asarray(y)
    fx, fy = np.broadcast_to(fx, x.shape), np.broadcast_to(fy, x.shape)
    return np.stack([x, y], -1).astype(np.int16), (fy * 32 + fx).astype(np.uint16)


def float_of(xy, frac):
    """the float maps whose conversion gives exactly these words (|coordinate| < 2^18: exact in float32)"""
    return (xy[..., 0].astype(np.float64) + (frac & 31) / 32.0).astype(np.float32), \
        (xy[..., 1].astype(np.float64) + (frac >> 5) / 32.0).astype(np.float32)


def hand_maps(name, w, h, sw, sh, seed=0):
    """the hand-made maps of the remap tests -> (xy, frac)"""
    j, i = np.meshgrid(np.arange(w), np.arange(h))
    rng = np.random.default_rng(seed)
    if name == "identity":
        return words(j, i)
    if name == "shift":
        return words(j + 2, i - 1)
    if name == "fractions":          # every one of the 1024 fraction pairs: w = h = 32
        return words(j % max(sw - 1, 1), i % max(sh - 1, 1), j % 32, i % 32)
    if name == "transpose":          # no locality along a row
        return words(i % sw, j % sh, 7, 19)
    if name == "permutation":
        p = rng.permutation(w * h).reshape(h, w)
        return words(p % sw, (p // sw) % sh, rng.integers(0, 32, (h, w)), rng.integers(0, 32, (h, w)))
    if name == "outside":            # every window fully outside, on all four sides and far away
        far = np.array([-2, sw, -32768, 32767])
        return words(far[(j + i) % 4], np.where((j + i) % 4 < 2, i % sh, far[(j + i) % 4]), 5, 9)
    if name == "half_outside":       # windows straddling each of the four sides, and the corners
        return words(np.where(j % 3 == 0, -1, np.where(j % 3 == 1, sw - 1, j % max(sw - 1, 1))),
                     np.where(i % 3 == 0, -1, np.where(i % 3 == 1, sh - 1, i % max(sh - 1, 1))), 13, 21)
    if name == "one_tap_inside":     # three taps outside at the bottom-right corner, two on the edges, and a straddling quad: pixels 0..2 of
        x = np.where(j % 4 == 3, sw - 1, j % max(sw - 1, 1))  # a quad inside, pixel 3 on the right edge
        return words(x, np.where(i % 3 == 2, sh - 1, i % max(sh - 1, 1)), 17, 3)
    if name == "random":             # anything, far outside included
        return words(rng.integers(-3, sw + 3, (h, w)), rng.integers(-3, sh + 3, (h, w)), rng.integers(0, 32, (h, w)),
                     rng.integers(0, 32, (h, w)))
    raise KeyError(name)


HAND_MAPS = ["identity", "shift", "fractions", "transpose", "permutation", "outside", "half_outside", "one_tap_inside", "random"]

# values at every boundary of the fixed-point conversion (N11, N12, N15), as float32 map entries
BOUNDARY = np.array([0.0, 1 / 64, 3 / 64, 5 / 64, -1 / 64, -3 / 64, 1 / 32, -1 / 32, -0.5, -1.0, -1 - 1 / 64, 0.484375, 0.515625, 7.984375,
                     32766.99, 32767.0, 32767.5, 32768.0, 40000.0, -32768.0, -32768.5, -32769.0, -40000.0, 6.7e7, 67108863.0, 67108864.0,
                     -67108864.0, -67108868.0, 1e12, -1e12, 3e38, -3e38, np.nan, np.inf, -np.inf], np.float32)


def ramp(sw, sh):
    """the integer-rounded ramp 0.25 x + 0.25 y + 20, saturated at 255 (it reaches 327 in the far corner of 752 x 480), and the
    function itself"""
    j, i = np.meshgrid(np.arange(sw, dtype=np.float64), np.arange(sh, dtype=np.float64))
    f = lambda x, y: 0.25 * x + 0.25 * y + 20
    return np.clip(np.rint(f(j, i)), 0, 255).astype(np.uint8), f


# ---- the composition chain: render with the rectified cameras -> warp to the raw rig -> rectify -> SGBM ------------------------
# A mild rig (k1 = -0.1: the five-iteration inverse is exact to 0.003 px, tests/test_rectify_numpy.py) with a baseline of 0.3 m, so
# that the scene's depths of 2 m and more give disparities below 32 at a focal length near 190.
COMPOSE_RIG = (_K(210.0, 211.0, 158.0, 101.0), [-0.10, 0.02, 0.0003, -0.0002], _K(209.0, 210.5, 163.0, 98.0),
               [-0.11, 0.018, -0.0002, 0.0003], (320, 200), Rot.from_rotvec([0.004, -0.012, 0.003]).as_matrix(),
               np.array([-0.3, 0.001, -0.002]))
COMPOSE_NUM_DISPARITIES = 32
COMPOSE_AGREE = 16   # |difference| of two disparities x 16 that counts as agreement: one pixel
# The share of pixels, among those valid in both disparity maps, on which the map of the warped-and-rectified pair agrees with the
# map of the pair that was never warped, measured on the CPU restatement of the whole chain (rectify_numpy.remap, sgbm_numpy.sgbm):
#     python tests/rectify_fixtures.py
# -> "compose: 53237 pixels valid in both maps, agreeing share 0.9688".  Two bilinear passes blur, so the maps are not equal and the
# share cannot be derived; the GPU test asserts the GPU chain's disagreeing share against this one plus one percentage point.
COMPOSE_SHARE = 0.9688


@functools.lru_cache(maxsize=None)
def compose_images():
    """-> (left, right: the grey pair rendered with the rectified cameras; raw_left, raw_right: the same pair warped to the raw rig
    through the restatement's inverse map; the rectification)"""
    from ros_stereo_slam_amd import synth

    K1, D1, K2, D2, size, R, T = COMPOSE_RIG
    rect = rn.stereo_rectify(K1, D1, K2, D2, size, R, T)
    R1, R2, P1, P2, _ = rect
    assert P1[0, 2] == P2[0, 2] and P1[1, 2] == P2[1, 2] and P2[0, 3] < 0   # one K for both rectified cameras, camera 2 to the right
    left, right, _ = synth.Scene().stereo(np.eye(3), np.zeros(3), K=(P1[0, 0], P1[1, 1], P1[0, 2], P1[1, 2]), size=size, channels=1,
                                          baseline=-P2[0, 3] / P2[0, 0])
    left, right = np.ascontiguousarray(left[..., 0]), np.ascontiguousarray(right[..., 0])
    j, i = np.meshgrid(np.arange(size[0], dtype=np.float32), np.arange(size[1], dtype=np.float32))
    raw = []
    for img, K, D, Ri, Pi in ((left, K1, D1, R1, P1), (right, K2, D2, R2, P2)):
        # where a raw pixel lies in the rectified image: undistortPoints(raw pixel, K, D, R_i, P_i)
        inv = rn.undistort_points(np.stack([j.ravel(), i.ravel()], 1), K, D, Ri, Pi).astype(np.float32)
        xy, frac = rn.float_maps(inv[:, 0].reshape(j.shape), inv[:, 1].reshape(j.shape))
        raw.append(rn.remap(img, xy, frac, 0))
    return left, right, raw[0], raw[1], rect


def compose_share(rectify, matcher):
    """rectify(raw_left, raw_right) -> the rectified pair; matcher(left, right) -> int16 disparities x 16 with min_disparity 1.
    -> (pixels valid in both maps, the share of them that agree within COMPOSE_AGREE)"""
    left, right, raw_left, raw_right, _ = compose_images()
    d_plain = np.asarray(matcher(left, right)).astype(np.int64)
    d_chain = np.asarray(matcher(*rectify(raw_left, raw_right))).astype(np.int64)
    both = (d_plain >= 16) & (d_chain >= 16)   # invalid is (min_disparity - 1) x 16 = 0
    return int(both.sum()), float((np.abs(d_plain - d_chain)[both] <= COMPOSE_AGREE).mean())


if __name__ == "__main__":
    import sgbm_numpy

    K1, D1, K2, D2, size, _, _ = COMPOSE_RIG
    R1, R2, P1, P2, _ = compose_images()[4]
    ml, mr = rn.init_undistort_rectify_map(K1, D1, R1, P1, size), rn.init_undistort_rectify_map(K2, D2, R2, P2, size)
    n, share = compose_share(lambda a, b: (rn.remap(a, *ml, 0), rn.remap(b, *mr, 0)),
                             lambda a, b: sgbm_numpy.sgbm(a, b, sgbm_numpy.Params(num_disparities=COMPOSE_NUM_DISPARITIES)))
    print(f"compose: {n} pixels valid in both maps, agreeing share {share:.4f}")
