"""tests/brief_numpy.py, the restatement the BRIEF kernels are held to, checked against things it shares no code with: integral
images in closed form, box sums by slicing, an image and a table whose bits are known by construction, the border filter on a
hand-made list (CPU only)."""
import numpy as np
import pytest

import brief_numpy as bn


def ring_table(nbytes=32):
    """a legal table that is no use for matching: test t compares (0, 0) with a point that walks round a square"""
    t = np.zeros((8 * nbytes, 4), np.int8)
    k = np.arange(8 * nbytes)
    t[:, 2], t[:, 3] = 1 + k % 7, 1 + k % 11
    return t


def test_integral_of_a_constant_and_of_a_ramp():
    h, w = 37, 53
    s = bn.integral(np.full((h, w), 7, np.uint8))
    y, x = np.mgrid[0:h + 1, 0:w + 1]
    assert s.dtype == np.int32 and s.shape == (h + 1, w + 1)
    assert np.array_equal(s, 7 * y * x)
    ramp = np.tile(np.arange(w, dtype=np.uint8), (h, 1))     # pixel (r, c) = c: the sum over c < x is x (x - 1) / 2
    assert np.array_equal(bn.integral(ramp), y * (x * (x - 1) // 2))
    assert np.all(bn.integral(ramp)[0] == 0) and np.all(bn.integral(ramp)[:, 0] == 0)
    full = bn.integral(np.full((376, 1241), 255, np.uint8))
    assert int(full[-1, -1]) == 255 * 376 * 1241


def test_grey_uses_the_integer_weights():
    img = np.random.default_rng(0).integers(0, 256, (9, 11, 3), dtype=np.uint8)
    want = [[(1868 * int(p[0]) + 9617 * int(p[1]) + 4899 * int(p[2]) + 8192) >> 14 for p in row] for row in img]
    assert np.array_equal(bn.to_grey(img), np.array(want, np.uint8))
    assert np.array_equal(bn.to_grey(img[..., 0]), img[..., 0])


def test_every_smoothed_sample_is_the_sum_of_its_9x9_block():
    rng = np.random.default_rng(1)
    grey = rng.integers(0, 256, (70, 90), dtype=np.uint8)
    s = bn.integral(grey)
    for iy, ix in [(4, 4), (65, 85), (4, 85), (65, 4), (30, 41), (28 - 24, 28 + 24)]:
        got = int(bn.smoothed(s, np.array([iy]), np.array([ix]))[0])
        assert got == int(grey[iy - 4:iy + 5, ix - 4:ix + 5].astype(np.int64).sum())
    iy, ix = rng.integers(4, 66, 200), rng.integers(4, 86, 200)
    want = [int(grey[a - 4:a + 5, b - 4:b + 5].astype(np.int64).sum()) for a, b in zip(iy, ix)]
    assert np.array_equal(bn.smoothed(s, iy, ix), want)


def test_bits_of_a_step_edge_are_known_by_construction():
    """left half 0, right half 200, the key point ON the edge column: a 9 x 9 box centred dx columns from it holds
    clip(dx + 5, 0, 9) bright columns, so S grows with dx between -5 and 4 and is flat outside"""
    h, w = 120, 160
    img = np.zeros((h, w), np.uint8)
    img[:, 80:] = 200
    xy = np.array([[80.0, 60.0]], np.float32)

    def bright(dx):
        return int(np.clip(dx + 5, 0, 9))

    rng = np.random.default_rng(2)
    table = np.zeros((256, 4), np.int8)
    while True:
        table[:, 0], table[:, 2] = rng.integers(-24, 25, 256), rng.integers(-24, 25, 256)
        table[:, 1], table[:, 3] = rng.integers(-8, 9, 256), rng.integers(-8, 9, 256)
        if not np.any((table[:, 0] == table[:, 2]) & (table[:, 1] == table[:, 3])):
            break
    table[0] = (0, -1, 0, 1)      # darker on the left: 1
    table[1] = (0, 1, 0, -1)      # 0
    table[2] = (5, -20, -5, -9)   # both boxes all dark: equal, so 0 (strict <)
    table[7] = (24, -24, -24, 24)  # the corners of the patch: 0 < 9 bright columns
    bits = np.array([bright(int(r[1])) < bright(int(r[3])) for r in table])
    desc, kept = bn.describe(img, xy, table, 32)
    assert list(kept) == [0] and desc.shape == (1, 32)
    assert bits[0] and not bits[1] and not bits[2] and bits[7]
    assert desc[0, 0] == 0b10000001 | (int(bits[3]) << 4) | (int(bits[4]) << 3) | (int(bits[5]) << 2) | (int(bits[6]) << 1)
    for t in range(256):           # MSB first inside a byte
        assert (int(desc[0, t // 8]) >> (7 - t % 8)) & 1 == int(bits[t]), t
    # the same edge with rows and columns exchanged exercises the y offsets
    desc_t, _ = bn.describe(np.ascontiguousarray(img.T), np.array([[60.0, 80.0]], np.float32), table[:, [1, 0, 3, 2]], 32)
    assert np.array_equal(desc_t, desc)
    # a three-channel image whose grey is that image gives the same bits
    assert np.array_equal(bn.describe(np.repeat(img[..., None], 3, axis=2), xy, table, 32)[0], desc)


@pytest.mark.parametrize("w", [101, 100])
def test_filter_on_a_hand_made_list(w):
    h = 90
    lo = np.nextafter(np.float32(27.5), np.float32(0))
    cases = [
        (27.5, 40.0, True),        # cvRound(27.5) = 28: half to even
        (28.5, 40.0, True),        # 28
        (float(lo), 40.0, False),  # just below 27.5 rounds to 27
        (27.49, 40.0, False),
        (28.0, 40.0, True),
        (w - 29.0, 40.0, True),    # the last admissible column
        (w - 28.0, 40.0, False),
        (40.0, 27.5, True), (40.0, 27.49, False), (40.0, h - 29.0, True), (40.0, h - 28.0, False),
        # w - 28.5: cvRound gives w - 29 for odd w (w - 28 is odd, w - 29 the even neighbour) and w - 28 for even w; where B4
        # keeps it, (int)(x + 0.5) = w - 28 would sample column w + 1 of the integral image: OURS-1 removes it
        (w - 28.5, 40.0, False),
        (40.0, h - 28.5, False),   # h = 90 is even: cvRound(61.5) = 62 = h - 28, B4 itself removes it
        (w - 29.5, 40.0, True),    # rounds to w - 30 or w - 29, centre w - 29
        (np.nan, 40.0, False), (40.0, np.inf, False), (-1e30, 40.0, False), (1e30, 40.0, False),
    ]
    xy = np.array([(a, b) for a, b, _ in cases], np.float32)
    assert list(bn.keep_mask(xy, w, h)) == [k for _, _, k in cases]
    # B4 alone keeps (w - 28.5, .) exactly when w is odd: that is the case OURS-1 exists for
    assert (np.rint(w - 28.5) < w - 28) == (w % 2 == 1)
    desc, kept = bn.describe(np.zeros((h, w), np.uint8), xy, ring_table(), 32)
    assert list(kept) == [i for i, c in enumerate(cases) if c[2]] and desc.shape == (len(kept), 32)


def test_small_images():
    pts = np.array([[28.0, 28.0], [27.6, 28.4], [29.0, 28.0], [28.0, 29.0], [28.5, 28.0], [28.0, 28.5]], np.float32)
    assert not bn.keep_mask(pts, 56, 200).any() and not bn.keep_mask(pts, 200, 56).any()
    # 57 x 57: Rect(28, 28, 1, 1) -- pixel (28, 28) alone; 28.5 rounds to 28 but its centre is 29: OURS-1
    assert list(bn.keep_mask(pts, 57, 57)) == [True, True, False, False, False, False]
    img = np.random.default_rng(3).integers(0, 256, (57, 57), dtype=np.uint8)
    desc, kept = bn.describe(img, pts, ring_table(), 32)     # every sample stays inside the 58 x 58 table
    assert list(kept) == [0, 1] and np.array_equal(desc[0], desc[1])
    assert bn.describe(img[:40, :40], pts, ring_table(), 32)[0].shape == (0, 32)


def test_half_integer_key_points_sample_the_next_pixel():
    """(int)(k + 0.5 + 0.5) = k + 1, the float just below gives k: the two descriptors are those of the integer key points"""
    rng = np.random.default_rng(4)
    img = rng.integers(0, 256, (100, 120), dtype=np.uint8)
    table = ring_table()
    k = np.float32(50.5)
    below = np.nextafter(k, np.float32(0))
    assert float(below) + 0.5 < 51.0
    d, kept = bn.describe(img, np.array([[k, 40.0], [below, 40.0], [51.0, 40.0], [50.0, 40.0]], np.float32), table, 32)
    assert len(kept) == 4
    assert np.array_equal(d[0], d[2]) and np.array_equal(d[1], d[3]) and not np.array_equal(d[0], d[1])
    assert list(bn.centres(np.array([[k, 40.0], [below, 40.0]], np.float32))[:, 0]) == [51.0, 50.0]


def test_table_rules():
    for bad in (np.full((256, 4), 25, np.int8), np.zeros((256, 4), np.int8), ring_table()[:255]):
        with pytest.raises(AssertionError):
            bn.check_table(bad, 32)
    for nbytes in (16, 32, 64):
        assert bn.check_table(ring_table(nbytes), nbytes).shape == (8 * nbytes, 4)
