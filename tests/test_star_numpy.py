"""tests/star_numpy.py against brute force that uses no integral image, and the proof from the restatement's own record that the
fixtures of tests/star_fixtures.py reach the branches they are named for (CPU only; tests/test_gpu_star.py compares the kernels
with the restatement on every one of them)."""
import numpy as np
import pytest

import star_fixtures as sf
import star_numpy as sn


def test_star_sums_against_direct_summation():
    """Every size index, every pixel of a 40 x 36 image: the image is zero-extended by 200 pixels (the largest star reaches 193), so
    that every pixel holds every star, and the direct sum adds the shifted image once per pixel of the square and of the diamond."""
    rng = np.random.default_rng(1)
    g = rng.integers(0, 256, (36, 40)).astype(np.int64)
    h, w = g.shape
    P = 200
    big = np.zeros((h + 2 * P, w + 2 * P), np.int64)
    big[P:P + h, P:P + w] = g
    for i in range(len(sn.SIZES0)):
        r, t = sn.SIZES0[i], sn.tilt(i)
        assert t + 1 <= P
        direct = np.zeros((h, w), np.int64)
        pixels = 0
        for dy in range(-t, t + 1):
            for dx in range(-t, t + 1):
                times = int(abs(dx) <= r and abs(dy) <= r) + int(abs(dx) + abs(dy) <= t)
                if times:
                    direct += times * big[P + dy:P + dy + h, P + dx:P + dx + w]
                    pixels += times
        assert pixels == sn.area(i)
        got = sn.star_sums(big, i, t)[P - t:P - t + h, P - t:P - t + w]
        assert got.shape == direct.shape and np.array_equal(got, direct), i
        assert direct.max() > 0


def test_response_at_the_largest_size_against_direct_summation():
    """max_size 128 on 470 x 430: all twelve patterns, border 192; a few interior pixels from direct sums, float32 step by step."""
    img = sf.huge()
    h, w = img.shape
    assert sn.layout(w, h, 128) == (12, 16, 192)
    resp, size, border, win = sn.responses(img, 128)
    g = img.astype(np.int64)
    F = np.float32

    def star(i, x, y):
        r, t = sn.SIZES0[i], sn.tilt(i)
        return int(g[y - r:y + r + 1, x - r:x + r + 1].sum()) + sum(int(g[y + dy, x - (t - abs(dy)):x + (t - abs(dy)) + 1].sum())
                                                                     for dy in range(-t, t + 1))

    for x, y in ((192, 192), (277, 237), (200, 205), (262, 222), (232, 213), (215, 230)):
        best, bsz, bp = F(0), 0, -1
        for p in range(12):
            o, i = sn.PAIRS[p]
            inner = star(i, x, y)
            outer = star(o, x, y) - inner
            r = F(F(inner) * (F(1) / F(sn.area(i)))) - F(F(outer) * (F(1) / F(sn.area(o) - sn.area(i))))
            if abs(r) > abs(best):
                best, bsz, bp = r, sn.SIZES0[o], p
        assert resp[y, x] == best and size[y, x] == bsz and win[y, x] == bp, (x, y)
    assert {9, 10, 11} <= set(np.unique(win).tolist())          # the last three patterns win somewhere


def test_cone_tables_at_their_edges():
    """The entries the diamonds read at the first and last columns: apex x = -1 and x = w - 1, every row."""
    rng = np.random.default_rng(2)
    g = rng.integers(0, 256, (9, 7)).astype(np.int64)
    h, w = g.shape
    big = np.zeros((h + 40, w + 40), np.int64)
    big[20:20 + h, 20:20 + w] = g
    _, even, odd = sn.tables(g)
    assert not even[0].any() and not odd[0].any()
    for y in range(h):
        for x in range(-1, w):
            e = sum(big[20 + yy, 20 + x - (y - yy):20 + x + (y - yy) + 1].sum() for yy in range(y + 1))
            o = sum(big[20 + yy, 20 + x - (y - yy):20 + x + (y - yy) + 2].sum() for yy in range(y + 1))
            assert even[y + 1, x + 1] == e and odd[y + 1, x + 1] == o, (x, y)


def test_areas_are_pixel_counts():
    for i in range(len(sn.SIZES0)):
        r, t = sn.SIZES0[i], sn.tilt(i)
        n = 2 * t + 3
        y, x = np.mgrid[-n:n + 1, -n:n + 1]
        count = int(((abs(x) <= r) & (abs(y) <= r)).sum() + (abs(x) + abs(y) <= t).sum())
        assert sn.area(i) == count


def literal_layout(w, h, max_size):
    sizes0 = [1, 2, 3, 4, 6, 8, 11, 12, 16, 22, 23, 32, 45, 46, 64, 90, 128]
    pairs = [[1, 0], [3, 1], [4, 2], [5, 3], [7, 4], [8, 5], [9, 6], [11, 8], [13, 10], [14, 11], [15, 12], [16, 14]]
    t = lambda i: sizes0[i] + sizes0[i] // 2
    n = 0
    while True:
        if not n < 12:
            break
        if not sizes0[pairs[n][0]] < max_size:
            break
        if not (n + 1 == 12 or t(pairs[n + 1][0]) < min(w, h)):
            break
        n = n + 1
    npatterns = min(n + 1, 12)
    max_idx = pairs[npatterns - 1][0]
    return npatterns, max_idx, t(max_idx)


def test_pattern_count():
    for size in (7, 13, 70, 139, 400):
        for max_size in range(3, 129):
            assert sn.layout(size, size, max_size) == literal_layout(size, size, max_size)
            assert sn.layout(size, 5000, max_size) == sn.layout(5000, size, max_size) == literal_layout(size, size, max_size)
    assert sn.layout(1241, 376, 45) == (9, 13, 69)
    assert sn.layout(5000, 5000, 128) == (12, 16, 192)


def test_response_plane_against_direct_summation():
    """One fixture, every interior pixel: patterns from direct sums, float32 step by step."""
    img, prm = sf.case("blobs")
    resp, size, border, win = sn.responses(img, prm["max_size"])
    g = img.astype(np.int64)
    h, w = g.shape
    npat = sn.layout(w, h, prm["max_size"])[0]
    assert not resp[:border].any() and not resp[:, :border].any() and not resp[h - border:].any() and not resp[:, w - border:].any()

    def star(i, x, y):
        r, t = sn.SIZES0[i], sn.tilt(i)
        return int(g[y - r:y + r + 1, x - r:x + r + 1].sum()) + sum(int(g[y + dy, x - (t - abs(dy)):x + (t - abs(dy)) + 1].sum())
                                                                     for dy in range(-t, t + 1))

    F = np.float32
    for y in range(border, h - border, 3):
        for x in range(border, w - border, 3):
            best, bsz = F(0), 0
            for p in range(npat):
                o, i = sn.PAIRS[p]
                inner = star(i, x, y)
                outer = star(o, x, y) - inner
                r = F(F(inner) * (F(1) / F(sn.area(i)))) - F(F(outer) * (F(1) / F(sn.area(o) - sn.area(i))))
                if abs(r) > abs(best):
                    best, bsz = r, sn.SIZES0[o]
            assert resp[y, x] == best and size[y, x] == bsz, (x, y)


RECORDS = {}


def record(name):
    if name not in RECORDS:
        img, prm = sf.case(name)
        rec = {}
        out = sn.detect(img, record=rec, **prm)
        RECORDS[name] = (rec, out)
    return RECORDS[name]


def test_every_fixture_reaches_its_branch():
    assert record("blobs")[0]["max_kept"] >= 2 and record("blobs")[0]["min_kept"] >= 2
    assert len(set(record("blobs")[1][1].tolist())) >= 3                      # several radii: several sizes
    assert record("bar")[0]["line_projected"] >= 1
    assert record("ramp_blob")[0]["line_binarized"] >= 1
    assert record("twins")[0]["neighbourhood_equal"] >= 1
    assert record("small")[0]["size_rule"] >= 1
    assert record("flat")[0]["candidates"] == 0 and not record("flat")[0]["patterns_won"]
    assert record("noise")[0]["candidates"] >= 100 and len(record("noise")[1][0]) >= 1
    assert len(record("large")[1][0]) >= 1
    assert len(record("colour")[1][0]) >= 1
    assert len(record("huge")[1][0]) >= 1 and {9, 10, 11} <= record("huge")[0]["patterns_won"]
    for name in sf.CASES:
        rec, (xy, size, resp) = record(name)
        assert rec["max_kept"] + rec["min_kept"] == len(xy) == len(size) == len(resp)
        assert rec["candidates"] == len(xy) + rec["neighbourhood"] + rec["size_rule"] + rec["line_projected"] + rec["line_binarized"]
        assert (size >= 4).all() and (np.abs(resp) > sf.case(name)[1].get("response_threshold", 30)).all()


def test_nothing_is_vacuous_across_the_set():
    total = {}
    won = {}
    for name in sf.CASES:
        rec, _ = record(name)
        for k, v in rec.items():
            if k != "patterns_won":
                total[k] = total.get(k, 0) + int(v)
        img, prm = sf.case(name)
        npat = sn.layout(img.shape[1], img.shape[0], prm.get("max_size", 45))[0]
        won.setdefault(npat, set()).update(rec["patterns_won"])
    for k in ("max_kept", "min_kept", "neighbourhood", "size_rule", "line_projected", "line_binarized"):
        assert total[k] >= 1, k
    assert set(won) == {6, 9, 12}
    assert set().union(*won.values()) == set(range(12))                            # every pattern index in use wins somewhere


def test_small_images_and_orders():
    for w, h in ((1, 1), (6, 6), (7, 6), (6, 40)):
        img = np.random.default_rng(w * 100 + h).integers(0, 256, (h, w), dtype=np.uint8)
        xy, size, resp = sn.detect(img, max_size=4, response_threshold=0)
        assert xy.shape == (0, 2) and not len(size) and not len(resp)
    # row-major tiles, a tile's maximum before its minimum
    img, prm = sf.case("noise")
    xy, _, resp = sn.detect(img, **prm)
    border, step = 24, 3
    key = [((int(y) - border) // step, (int(x) - border) // step, r < 0) for (x, y), r in zip(xy, resp)]
    assert key == sorted(key) and len(set(key)) == len(key)


@pytest.mark.parametrize("nonmax", [1, 3, 5, 7])
def test_no_two_extrema_of_one_sign_within_the_neighbourhood(nonmax):
    img, prm = sf.case("noise")
    prm.update(suppress_nonmax_size=nonmax, response_threshold=4)
    xy, _, resp = sn.detect(img, **prm)
    assert len(xy) >= 2
    d = nonmax // 2
    for sign in (1, -1):
        pts = xy[resp * sign > 0]
        gap = np.abs(pts[:, None, :] - pts[None, :, :]).max(-1)
        gap[np.arange(len(pts)), np.arange(len(pts))] = 1e9
        assert len(pts) < 2 or gap.min() > d
