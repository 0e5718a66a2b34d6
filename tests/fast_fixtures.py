"""Seeded, small images for the FAST tests, each named for the branch of the detector it reaches; tests/test_fast_numpy.py proves
from the restatement that it does.  The largest is 160 x 120."""
import numpy as np


def noise(w, h, seed, channels=1):
    rng = np.random.default_rng(seed)
    shape = (h, w) if channels == 1 else (h, w, channels)
    return rng.integers(0, 256, shape, dtype=np.uint8)


def blocks(w, h, seed, cell=7, levels=6, grain=8):
    """Random piecewise-constant cells of a few grey levels under a little noise: many corners, many of them with equal scores,
    and enough of them strict maxima."""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, levels, ((h + cell - 1) // cell, (w + cell - 1) // cell))
    img = np.kron(coarse, np.ones((cell, cell), np.int64))[:h, :w] * (225 // (levels - 1))
    return (img + rng.integers(0, grain, (h, w))).astype(np.uint8)


def dots(w, h, points, ground=100, peak=255):
    """Single bright pixels on a flat ground: each fires alone (its whole ring is darker), nothing else does."""
    img = np.full((h, w), ground, np.uint8)
    for x, y in points:
        img[y, x] = peak
    return img


def checkerboard(w, h, cell=5):
    ys, xs = np.mgrid[0:h, 0:w]
    return (((xs // cell + ys // cell) & 1) * 255).astype(np.uint8)


def edge_dots(w=40, h=30):
    """Corners on the first and last interior rows and columns only (x = 3, y = 3, x = w - 4, y = h - 4)."""
    pts = [(3, 3), (w - 4, 3), (3, h - 4), (w - 4, h - 4), (11, 3), (3, 12), (w - 4, 17), (22, h - 4)]
    return dots(w, h, pts), pts


def one_corner_7x7():
    return dots(7, 7, [(3, 3)], ground=50, peak=200)


def tied_pair(w=20, h=14):
    """Two adjacent bright pixels with equal scores, and further right a horizontal plateau of three."""
    img = np.full((h, w), 60, np.uint8)
    img[6, 5:7] = 220
    img[6, 12:15] = 220
    return img


def all_fixtures():
    return {
        "noise_64x48": noise(64, 48, 11),
        "flat_40x30": np.full((30, 40), 128, np.uint8),
        "one_corner_7x7": one_corner_7x7(),
        "no_interior_20x6": noise(20, 6, 12),
        "no_interior_6x20": noise(6, 20, 13),
        "odd_67x35": noise(67, 35, 14),
        "partial_tiles_75x41": noise(75, 41, 20),
        "checkerboard_48x40": checkerboard(48, 40),
        "bgr_50x37": noise(50, 37, 15, channels=3),
        "bgr_blocks_64x40": np.stack([blocks(64, 40, 16), blocks(64, 40, 17), blocks(64, 40, 18)], axis=-1),
        "edge_dots_40x30": edge_dots()[0],
        "tied_pair_20x14": tied_pair(),
        "blocks_160x120": blocks(160, 120, 19),
    }
