"""Images and parameter sets for the goodFeaturesToTrack tests, each named for the branch of tests/gftt_numpy.py it reaches;
``reaches`` proves from the restatement's record (and result) that it does.  The largest image is 160 x 96."""
import functools

import numpy as np

import gftt_numpy as gn


def noise(w, h, seed, channels=1):
    rng = np.random.default_rng(seed)
    shape = (h, w) if channels == 1 else (h, w, channels)
    return rng.integers(0, 256, shape, dtype=np.uint8)


def blocks(w, h, seed, cell=7, levels=6, grain=8):
    """Random flat cells with a little grain: corners at the cell crossings, edges (min-eigenvalue near 0) between them."""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, levels, ((h + cell - 1) // cell, (w + cell - 1) // cell)) * (200 // levels) + 20
    img = np.kron(coarse, np.ones((cell, cell), np.int64))[:h, :w]
    return np.clip(img + rng.integers(0, grain, (h, w)), 0, 255).astype(np.uint8)


def dots(w, h, points, ground=100):
    """Isolated pixels (x, y, value) on a flat ground"""
    img = np.full((h, w), ground, np.uint8)
    for x, y, v in points:
        img[y, x] = v
    return img


def squares(w, h, points, ground=60, value=220):
    """2 x 2 squares with their top-left pixel at (x, y): by symmetry the four pixels share one measure"""
    img = np.full((h, w), ground, np.uint8)
    for x, y in points:
        img[y:y + 2, x:x + 2] = value
    return img


def ramp_of_dots(w=160, h=24, step=6, first=250, drop=9):
    """Dots of falling brightness step pixels apart on one row: with min_distance between step and 2 step every dot waits for its
    brighter neighbour, a dependency chain as long as the row"""
    return dots(w, h, [(6 + step * k, h // 2, first - drop * k) for k in range((w - 12) // step) if first - drop * k > 110])


def dot_lattice(n, step=6, per_row=70):
    """n dots of 50 different brightnesses on a lattice: with block size 3 and quality 0.1 exactly n candidates, many of them equal"""
    rows = (n + per_row - 1) // per_row
    return dots(step * per_row + 6, step * rows + 6, [(4 + step * (k % per_row), 4 + step * (k // per_row), 200 + k % 50) for k in range(n)])


def case(img, reaches, mask=None, **params):
    return dict(img=img, mask=mask, params=params, reaches=reaches)


def _interior(w, h):
    """A mask of the pixels a corner may lie on: the maximum the cut is taken from is then a candidate's"""
    mask = np.zeros((h, w), np.uint8)
    mask[1:-1, 1:-1] = 1
    return mask


def _hide_maximum(img):
    eig = gn.response(img)
    y, x = np.unravel_index(np.argmax(eig), eig.shape)
    mask = np.full(eig.shape, 255, np.uint8)
    mask[max(y - 3, 0):y + 4, max(x - 3, 0):x + 4] = 0
    return mask, float(eig.max())


@functools.lru_cache(maxsize=None)
def all_cases():
    """name -> dict(img, mask, params, reaches(record, xy, response) -> bool)"""
    base = noise(96, 64, 1)
    c = {}
    c["tie_inside_min_distance"] = case(dots(40, 24, [(12, 10, 250), (18, 10, 250)]),
                                        lambda r, xy, v: r["ties"] >= 1 and r["n_accepted"] == 1 and r["n_candidates"] >= 2
                                        and tuple(xy[0]) == (18.0, 10.0), min_distance=10.0, quality_level=0.5)
    c["plateau"] = case(squares(48, 32, [(10, 8), (30, 20)]), lambda r, xy, v: r["plateau"] and r["ties"] >= 3,
                        min_distance=0.0, quality_level=0.5)
    c["plateau_min_distance"] = case(squares(48, 32, [(10, 8), (30, 20)]),
                                     lambda r, xy, v: r["plateau"] and r["n_accepted"] == 2 and r["n_candidates"] == 8 and r["cell"] == 2,
                                     min_distance=1.5, quality_level=0.5)
    c["border_columns"] = case(noise(50, 37, 3), lambda r, xy, v: r["x_min"] == 1 and r["x_max"] == 48, min_distance=0.0,
                               max_corners=0)
    c["flat"] = case(np.full((30, 40), 77, np.uint8), lambda r, xy, v: r["max_val"] == 0.0 and len(xy) == 0)
    # G7's comparison is strict: at quality 1 the cut IS the maximum and nothing is above it
    c["quality_one"] = case(base, lambda r, xy, v: r["max_val"] > 0 and r["threshold"] == r["max_val"] and r["n_candidates"] == 0,
                            quality_level=1.0)
    c["quality_just_below_one"] = case(base, lambda r, xy, v: 1 <= r["n_candidates"] <= 3 and v[0] == np.float32(r["max_val"]),
                                       mask=_interior(96, 64), quality_level=0.999)
    mask, full_max = _hide_maximum(base)
    c["mask_hides_maximum"] = case(base, lambda r, xy, v: 0 < r["max_val"] < full_max and len(xy) > 0, mask=mask, max_corners=0)
    c["mask_hides_everything"] = case(base, lambda r, xy, v: r["max_val"] == 0.0 and len(xy) == 0, mask=np.zeros((64, 96), np.uint8))
    for md in (0.0, 0.4, 1.0, 1.5, 2.5, 10.0, 500.0):
        def reaches(r, xy, v, md=md):
            if md < 1:
                return r["n_accepted"] == r["n_candidates"] > 50 and r["cell"] == 0
            if md == 500.0:
                return r["n_accepted"] == 1 and r["cell"] == 500
            if md < 2:                                        # strict 3 x 3 maxima are never neighbours
                return r["n_accepted"] == r["n_candidates"] > 50 and r["cell"] == round(md + 0.01)
            return 1 < r["n_accepted"] < r["n_candidates"] and r["cell"] == {1.0: 1, 1.5: 2, 2.5: 2, 10.0: 10}[md]
        c[f"min_distance_{md:g}"] = case(base, reaches, min_distance=md, max_corners=0)
    free = gn.detect(base, max_corners=0, min_distance=5.0)[2]["n_accepted"]
    for name, mc in (("zero", 0), ("one", 1), ("exact", free), ("one_fewer", free - 1)):
        c[f"max_corners_{name}"] = case(base, lambda r, xy, v, mc=mc: r["n_accepted_unbounded"] == free > 3
                                        and len(xy) == (mc if mc else free), min_distance=5.0, max_corners=mc)
    c["harris_negative"] = case(blocks(96, 64, 3), lambda r, xy, v: r["negative"] > 100 and len(xy) > 3 and (v > 0).all(),
                                use_harris=True, min_distance=3.0)
    c["harris_block5_bgr"] = case(noise(67, 35, 4, channels=3), lambda r, xy, v: len(xy) > 3, use_harris=True, block_size=5, k=0.06)
    c["three_by_three"] = case(noise(3, 3, 5), lambda r, xy, v: not r["too_small"] and r["n_candidates"] <= 1)
    c["two_by_five"] = case(noise(2, 5, 6), lambda r, xy, v: r["too_small"] and len(xy) == 0)
    c["selection_chain"] = case(ramp_of_dots(), lambda r, xy, v: r["rounds"] > 8 and 1 < r["n_accepted"] < r["n_candidates"],
                                min_distance=8.0, quality_level=0.05)
    c["block7_blocks"] = case(blocks(160, 96, 7), lambda r, xy, v: len(xy) > 3 and r["rounds"] > 2, block_size=7, min_distance=10.0)
    c["block31"] = case(noise(70, 40, 8), lambda r, xy, v: len(xy) >= 1, block_size=31, min_distance=3.0)
    return c


@functools.lru_cache(maxsize=None)
def expected(name):
    """The restatement's answer to a case, computed once"""
    k = all_cases()[name]
    return gn.detect(k["img"], mask=k["mask"], **k["params"])
