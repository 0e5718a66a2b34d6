"""Seeded, small inputs for the Star detector's tests: each is named for the branch of tests/star_numpy.py it is there to reach;
tests/test_star_numpy.py proves from the restatement's own record that it does.  CASES: name -> (image, parameters)."""
import numpy as np

W, H = 131, 97          # max_size 16: six patterns, border 24


def _blob(img, cx, cy, sigma, amp):
    h, w = img.shape
    y, x = np.mgrid[0:h, 0:w]
    img += amp * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2.0 * sigma * sigma))


def _u8(img):
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def blobs():
    """Gaussian blobs of both polarities at several radii."""
    img = np.full((H, W), 120.0)
    for k, (cx, cy, s) in enumerate([(32, 32, 1.5), (52, 34, 2.5), (75, 33, 4.0), (100, 36, 6.0), (34, 62, 6.0), (58, 64, 4.0),
                                     (80, 63, 2.5), (101, 65, 9.0)]):
        _blob(img, cx, cy, s, 110.0 if k % 2 == 0 else -110.0)
    return _u8(img)


def bar():
    """A long bright bar: its ridge is an extremum along one direction only."""
    img = np.full((H, W), 60.0)
    img[44:51, 10:121] = 220.0
    rng = np.random.default_rng(5)
    return _u8(img + rng.integers(0, 3, img.shape))


def ramp_blob():
    """A soft edge with blobs sitting on it: the response plane around them is two-dimensional, the plane of their size is a strip."""
    y, x = np.mgrid[0:H, 0:W]
    img = 40.0 + 170.0 / (1.0 + np.exp(-(x - 65.0) / 2.0))
    for cy in (34, 50, 66):
        _blob(img, 65, cy, 5.0, 60.0 if cy != 50 else -60.0)
    return _u8(img)


def twins():
    """Mirror images of one blob two pixels apart, in neighbouring tiles: equal responses remove each other."""
    img = np.full((H, W), 90.0)
    for cy in (30, 45, 60):
        for cx in (25, 28):           # the mirror axis is x = 26.5; tiles of 3 start at 24, 27
            img[cy - 2:cy + 3, cx - 0:cx + 1] = 230.0
    half = img[:, :27]
    img[:, 27:54] = half[:, ::-1]
    return _u8(img)


def small():
    """Blobs of a pixel or two whose best pattern is the first (outer size 2): below the smallest key point."""
    img = np.full((H, W), 100.0)
    for k, (cx, cy) in enumerate([(30, 30), (50, 40), (70, 50), (90, 60), (40, 66)]):
        _blob(img, cx, cy, 0.9, 150.0 if k % 2 == 0 else -100.0)
    return _u8(img)


def flat():
    return np.full((H, W), 137, np.uint8)


def noise():
    return np.random.default_rng(11).integers(0, 256, (H, W), dtype=np.uint8)


def large():
    """The default parameters (nine patterns, border 69) on 160 x 150: blobs wide enough for the outer sizes 22, 32 and 45."""
    img = np.full((150, 160), 128.0)
    _blob(img, 72, 72, 11.0, 100.0)
    _blob(img, 86, 77, 17.0, -90.0)
    _blob(img, 80, 74, 26.0, 60.0)
    rng = np.random.default_rng(3)
    return _u8(img + rng.normal(0, 2.0, img.shape))


def huge():
    """max_size 128 (twelve patterns, border 192) on 470 x 430, interior 86 x 46: blobs wide enough for the outer sizes 64, 90, 128."""
    img = np.full((430, 470), 128.0)
    _blob(img, 200, 205, 20.0, 110.0)
    _blob(img, 262, 222, 34.0, -100.0)
    _blob(img, 232, 213, 60.0, 60.0)
    rng = np.random.default_rng(9)
    return _u8(img + rng.normal(0, 2.0, img.shape))


def colour():
    """BGR: the three channels differ, so that the grey weights matter."""
    g = blobs().astype(np.float64)
    rng = np.random.default_rng(17)
    img = np.stack([g * 0.5 + 60, g, g * 0.8 + 10], -1) + rng.integers(0, 5, (H, W, 3))
    return _u8(img)


P16 = dict(max_size=16)
CASES = {
    "blobs": (blobs, P16),
    "bar": (bar, P16),
    "ramp_blob": (ramp_blob, P16),
    "twins": (twins, P16),
    "small": (small, dict(max_size=16, response_threshold=10)),
    "flat": (flat, P16),
    "noise": (noise, dict(max_size=16, response_threshold=12)),
    "large": (large, dict(response_threshold=6)),
    "colour": (colour, P16),
    "huge": (huge, dict(max_size=128, response_threshold=2)),
}


def case(name):
    make, prm = CASES[name]
    return make(), dict(prm)
