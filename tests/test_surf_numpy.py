"""The numpy restatement of SURF (tests/surf_numpy.py) against things known in closed form or by hand: the resized box
filters, det on a constant image, a straight edge and a step corner, Gaussian blobs, a 90 degree rotation, unit norm, the total
order of the sort and the drop of a key point too large for the image.  No GPU."""
from fractions import Fraction

import numpy as np

import surf_numpy as sn

f32 = np.float32


def exact_round(size, c, old=9):
    return int(round(Fraction(size * c, old)))   # Fraction rounds half to even; size * c / 9 is never a half (2 size c is even, 9 (2 k + 1) odd)


def test_resized_haar_corners():
    """octave 0 written out by hand (lobe = size / 3; the inner edges 2/9 and 7/9 of the size, rounded); every other size by exact
    rational arithmetic -- (float)size / 9 * c can never round differently because the exact value is never within 1/18 of a half"""
    hand = {9: (2, 3, 6, 7, 1, 4, 5, 8), 15: (3, 5, 10, 12, 2, 7, 8, 13), 21: (5, 7, 14, 16, 2, 9, 12, 19),
            27: (6, 9, 18, 21, 3, 12, 15, 24), 33: (7, 11, 22, 26, 4, 15, 18, 29)}
    for size, (c2, c3, c6, c7, c1, c4, c5, c8) in hand.items():
        dx = sn.resize_haar(sn.DX_S, 9, size)
        assert [r[:4] for r in dx] == [(0, c2, c3, c7), (c3, c2, c6, c7), (c6, c2, size, c7)]
        dy = sn.resize_haar(sn.DY_S, 9, size)
        assert [r[:4] for r in dy] == [(c2, 0, c7, c3), (c2, c3, c7, c6), (c2, c6, c7, size)]
        dxy = sn.resize_haar(sn.DXY_S, 9, size)
        assert [r[:4] for r in dxy] == [(c1, c1, c4, c4), (c5, c1, c8, c4), (c1, c5, c4, c8), (c5, c5, c8, c8)]
    sizes, steps, _, _ = sn.layers_layout(4096, 4096, 8, 8)
    assert sizes[:5] == [9, 15, 21, 27, 33] and sizes[10] == 18 and steps[10] == 2 and len(sizes) == 80
    for size in sorted(set(sizes)):
        for src in (sn.DX_S, sn.DY_S, sn.DXY_S):
            for row, got in zip(src, sn.resize_haar(src, 9, size)):
                want = tuple(exact_round(size, c) for c in row[:4])
                assert got[:4] == want
                assert got[4] == f32(row[4]) / (f32(want[2] - want[0]) * f32(want[3] - want[1]))
    # the gradient wavelets of the orientation stage, resized from 4
    assert [r[:4] for r in sn.resize_haar(sn.GDX_S, 4, 10)] == [(0, 0, 5, 10), (5, 0, 10, 10)]
    assert [r[:4] for r in sn.resize_haar(sn.GDY_S, 4, 6)] == [(0, 0, 6, 3), (0, 3, 6, 6)]


def test_det_on_constant_edge_and_corner():
    flat = np.full((48, 48), 137, np.uint8)
    det, trace = sn.layers(flat, 2, 3)
    assert all(not d.any() for d in det) and all(not t.any() for t in trace)
    # a straight unit edge: dyy and dxy vanish exactly (equal counts under weights w, -2 w, w), so det is zero
    edge = np.zeros((48, 48), np.uint8)
    edge[:, 23:] = 1
    det, trace = sn.layers(edge, 2, 3)
    assert all(not d.any() for d in det) and any(t.any() for t in trace)
    # a unit step corner in the middle of a 9-filter at origin (15, 15): ones at relative rows and columns >= 5.
    # Dx: boxes of 5 x 3 = 15 cells, weights 1/15, -2/15, 1/15, hold 0, 2 and 6 ones; Dy alike; Dxy: boxes of 9 cells, only the
    # last one (weight 1/9) is covered, by 9 ones.  dx = dy = 2/15, dxy = 1, det = 4/225 - 0.81
    corner = np.zeros((40, 40), np.uint8)
    corner[20:, 20:] = 1
    det, trace = sn.layers(corner, 1, 1)
    w15, w9 = f32(1) / f32(15), f32(1) / f32(9)
    dx = f32(np.float64(f32(0) * w15) + np.float64(f32(2) * (f32(-2) / f32(15))) + np.float64(f32(6) * w15))
    dxy = f32(np.float64(f32(9) * w9))
    assert det[0][19, 19] == dx * dx - f32(0.81) * dxy * dxy
    assert abs(float(det[0][19, 19]) - (4 / 225 - 0.81)) < 1e-6 and abs(float(trace[0][19, 19]) - 4 / 15) < 1e-6
    # stored at (i + margin, j + margin) with margin 4, and nothing outside the sampled square
    assert not det[0][:4].any() and not det[0][36:].any() and not det[0][:, :4].any() and not det[0][:, 36:].any()


def blob(sign):
    yy, xx = np.mgrid[0:64, 0:64]
    g = np.exp(-((xx - 32) ** 2 + (yy - 32) ** 2) / (2 * 16.0))
    return (40 + 200 * g).astype(np.uint8) if sign > 0 else (240 - 200 * g).astype(np.uint8)


def test_gaussian_blobs():
    """A blob of sigma 4 gives one key point within a pixel of its centre.  Its size is the interpolated maximum over the layers:
    it lies between the sizes next to the layer whose det is largest at the centre, and its scale s = 1.2 size / 9 within 1.5 px of
    sigma (the box filters answer a Gaussian blob most strongly at s near 0.75 sigma: 22 px here, between layers 21 and 27)."""
    laps = []
    for sign in (1, -1):
        img = blob(sign)
        r = sn.extract(img)
        assert len(r["xy"]) == 1
        assert np.abs(r["xy"][0] - 32).max() <= 1
        det, _ = sn.layers(img)
        sizes, steps, _, _ = sn.layers_layout(64, 64)
        centre = [det[k][32 // steps[k], 32 // steps[k]] for k in range(5)]
        best = sizes[int(np.argmax(centre))]
        assert best - 6 <= r["size"][0] <= best + 6
        assert abs(float(sn.scale_of(r["size"][0])) - 4.0) < 1.5
        assert abs(np.linalg.norm(r["desc"][0]) - 1) < 1e-6
        laps.append(int(r["laplacian"][0]))
    assert laps == [-1, 1]


def scene():
    yy, xx = np.mgrid[0:96, 0:96].astype(float)
    b = lambda cx, cy, s: np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * s * s))   # noqa: E731
    return (60 + 150 * b(48, 48, 4) - 50 * b(60, 44, 6) + 30 * b(40, 58, 5)).clip(0, 255).astype(np.uint8)


def test_rotation_by_90_degrees():
    """np.rot90 maps the pixel lattice onto itself, so every box sum recurs and the angle turns by a quarter turn (270 in
    fastAtan2's sense, image y down) -- bar: 5 degrees, the search step.  The descriptor window is then sampled along turned axes
    whose sin / cos differ by float rounding; a sample can change by one grey level.  Bar on the cosine distance: 1e-3 (a 4 %
    relative change, far above such effects, far below unrelated descriptors at 0.3 and more).  Measured on this restatement:
    turn 270.000 degrees, cosine distance 0.0 for the strongest key point, at most 6e-8 over all."""
    img = scene()
    a, b = sn.extract(img), sn.extract(np.ascontiguousarray(np.rot90(img)))
    assert len(a["xy"]) == len(b["xy"]) >= 3
    assert np.array_equal(a["response"], b["response"]) and np.array_equal(a["size"], b["size"])
    # (x, y) -> (y, w - 1 - x)
    assert np.allclose(b["xy"][:, 0], a["xy"][:, 1], atol=1e-3) and np.allclose(b["xy"][:, 1], 95 - a["xy"][:, 0], atol=1e-3)
    turn = (b["angle"] - a["angle"]) % 360
    assert np.abs(turn - 270).max() <= 5
    cosd = 1 - np.sum(a["desc"] * b["desc"], axis=1)
    print(f"rot90: turn {turn}, cosine distances {cosd}")
    assert np.abs(cosd).max() <= 1e-3
    assert np.abs(np.linalg.norm(a["desc"], axis=1) - 1).max() < 1e-6


def test_sort_is_a_total_order_on_equal_responses():
    rng = np.random.default_rng(0)
    n = 64
    resp = np.repeat(f32(500), n)
    size = np.repeat(f32(21), n)
    octave = np.zeros(n, np.int32)
    y = np.repeat(f32(10.5), n)
    x = np.repeat(f32(7.5), n)
    layer, row, col = rng.integers(1, 4, n), rng.integers(0, 8, n), np.arange(n) % 8
    # planted: equal in every field of KeypointGreater, distinct only in the sample
    seen = set()
    keep = [k for k in range(n) if (layer[k], row[k], col[k]) not in seen and not seen.add((layer[k], row[k], col[k]))]
    args = [v[keep] for v in (resp, size, octave, y, x, layer, row, col)]
    base = sn.sort_order(*args)
    for _ in range(5):
        p = rng.permutation(len(keep))
        got = sn.sort_order(*[v[p] for v in args])
        assert [tuple(int(v[p][k]) for v in args[5:]) for k in got] == [tuple(int(v[k]) for v in args[5:]) for k in base]
    order = [tuple(int(v[k]) for v in args[5:]) for k in base]
    assert order == sorted(order)
    # and KeypointGreater itself: response, size, octave descending, y descending, x ascending
    resp2 = np.array([1, 2, 2, 2, 2, 2], f32)
    size2 = np.array([9, 9, 15, 15, 15, 15], f32)
    oct2 = np.array([0, 0, 0, 1, 1, 1], np.int32)
    y2 = np.array([0, 0, 0, 1, 2, 2], f32)
    x2 = np.array([0, 0, 0, 0, 5, 4], f32)
    z = np.zeros(6, np.int32)
    assert sn.sort_order(resp2, size2, oct2, y2, x2, z, z, z) == [5, 4, 3, 2, 1, 0]


def test_a_key_point_too_large_for_the_image_is_dropped():
    img = blob(1)
    xy = np.array([[32, 32], [32, 32], [32, 32], [2, 2], [32, 32]], f32)
    size = np.array([22, 250, 120, 120, 5], f32)   # grad_wav_size 12, 134 (> 65), 64, 64 (no sample inside at (2, 2)), a window below 21
    angle, desc, kept = sn.compute(img, xy, size)
    assert kept.tolist() == [1, 0, 1, 0, 0]
    assert angle[1] == -1 and not desc[1].any() and angle[3] == -1 and angle[4] == -1
    assert abs(np.linalg.norm(desc[2]) - 1) < 1e-6
    # upright: only the size test applies
    angle, desc, kept = sn.compute(img, xy, size, upright=1)
    assert kept.tolist() == [1, 0, 1, 1, 0] and angle[0] == 270
    # the detector never returns one: an 8 x 8 image has no layer that fits
    assert len(sn.extract(np.arange(64, dtype=np.uint8).reshape(8, 8))["xy"]) == 0
