"""tests/fast_numpy.py, the restatement the FAST kernels are held to, pinned against things that do not depend on it: the ORB
restatement's score plane (tests/orb_numpy.py, written for the extractor), a brute force over every threshold, hand-made
suppression cases, and for every fixture of tests/fast_fixtures.py the proof that it reaches the branch it is named for."""
import numpy as np
import pytest

import fast_fixtures as ff
import fast_numpy as fn
import orb_numpy as on

FIX = ff.all_fixtures()


def test_ring_is_the_orb_restatements_ring():
    assert fn.RING == on.RING
    assert len(set(fn.RING)) == 16 and all(round(np.hypot(dx, dy)) == 3 for dx, dy in fn.RING)


def test_gray_is_the_extractors_conversion():
    img = FIX["bgr_50x37"]
    assert np.array_equal(fn.to_gray(img), on.to_gray(img))
    assert np.array_equal(fn.to_gray(FIX["noise_64x48"]), FIX["noise_64x48"])


@pytest.mark.parametrize("name", sorted(FIX))
@pytest.mark.parametrize("t", [0, 1, 10, 40, 255])
def test_score_plane_equals_the_orb_restatements(name, t):
    g = fn.to_gray(FIX[name])
    h, w = g.shape
    if h < 7 or w < 7:
        assert not fn.score_image(g, t).any() and not fn.fires(g, t).any()   # orb_numpy does not take an image without an interior
        return
    assert np.array_equal(fn.score_image(g, t), on.fast_score_image(g, t))
    assert np.array_equal(fn.fires(g, t), on.fast_fires(g, t))


def test_brute_force_over_every_threshold():
    g = ff.noise(24, 20, 5)
    fires0, score0 = fn.fires(g, 0), fn.score_image(g, 0).astype(int)
    largest = np.full(g.shape, -1)
    for t in range(256):
        f = fn.fires(g, t)
        assert np.array_equal(f, fires0 & (score0 >= t)), t
        assert np.array_equal(f, on.fast_fires(g, t)), t
        largest[f] = t
        sc = fn.score_image(g, t).astype(int)
        assert np.array_equal(sc, np.where(f, score0, 0)), t
    # the score is the largest threshold at which the pixel still fires
    assert fires0.sum() > 20
    assert np.array_equal(largest[fires0], score0[fires0])
    assert (largest[~fires0] == -1).all()


def test_threshold_is_clamped():
    g = FIX["noise_64x48"]
    assert np.array_equal(fn.fires(g, -5), fn.fires(g, 0))
    assert np.array_equal(fn.fires(g, 300), fn.fires(g, 255)) and not fn.fires(g, 255).any()


# ------------------------------------------------------------------------------------------------------------- suppression
def test_corners_on_the_first_and_last_interior_rows_and_columns():
    img, pts = ff.edge_dots()
    h, w = img.shape
    xy, resp, score = fn.fast_detect(img, 10, True)
    assert sorted(map(tuple, xy.astype(int).tolist())) == sorted(pts)
    assert {x for x, y in pts} >= {3, w - 4} and {y for x, y in pts} >= {3, h - 4}
    assert (resp == 154).all()                                  # 255 - 100 - 1: neighbours outside the interior count 0
    assert not score[:3].any() and not score[-3:].any() and not score[:, :3].any() and not score[:, -3:].any()


def test_equal_neighbours_remove_each_other():
    img = ff.tied_pair()
    f, s = fn.fires(img, 10), fn.score_image(img, 10)
    assert f[6, 5] and f[6, 6] and s[6, 5] == s[6, 6] == 159
    assert f[6, 12] and f[6, 13] and f[6, 14] and s[6, 12] == s[6, 13] == s[6, 14] == 159
    assert f.sum() == 5
    xy, resp, _ = fn.fast_detect(img, 10, True)
    assert len(xy) == 0
    xy, resp, _ = fn.fast_detect(img, 10, False)
    assert len(xy) == 5 and not resp.any()


def test_suppress_on_hand_made_planes():
    score = np.zeros((9, 9), np.uint8)
    fired = np.zeros((9, 9), bool)
    for (y, x), v in {(3, 3): 9, (3, 4): 7, (5, 5): 7, (4, 4): 0}.items():
        fired[y, x], score[y, x] = True, v
    keep = fn.suppress(fired, score)
    assert keep[3, 3] and not keep[3, 4] and keep[5, 5]
    assert not keep[4, 4]                                       # a corner that scores 0 is never strictly above a 0
    assert keep.sum() == 2


def test_order_is_row_major():
    for name in ("noise_64x48", "blocks_160x120"):
        for nonmax in (True, False):
            xy, _, _ = fn.fast_detect(FIX[name], 1, nonmax)
            key = xy[:, 1].astype(np.int64) * 100000 + xy[:, 0].astype(np.int64)
            assert len(key) > 10 and (np.diff(key) > 0).all()


# ------------------------------------------------------------------------------------------------------------- retainBest
def tie_budget(resp):
    """A budget whose cut lands on a tie: the k-th and the (k + 1)-th largest responses are equal."""
    s = np.sort(resp)[::-1]
    ks = [k for k in range(1, len(s)) if s[k - 1] == s[k]]
    assert ks
    return ks[len(ks) // 2]


def test_retain_best_keeps_ties_and_order_and_can_exceed_the_budget():
    xy = np.arange(14, dtype=np.float32).reshape(7, 2)
    resp = np.array([5, 9, 5, 1, 7, 5, 2], np.float32)
    kxy, kr = fn.retain_best(xy, resp, 3)                      # third largest is 5: three fives come along
    assert kr.tolist() == [5, 9, 5, 7, 5] and np.array_equal(kxy, xy[[0, 1, 2, 4, 5]])
    assert fn.retain_best(xy, resp, 1)[1].tolist() == [9]
    assert fn.retain_best(xy, resp, 7)[1].tolist() == resp.tolist()
    assert fn.retain_best(xy, resp, 0)[1].tolist() == resp.tolist()          # 0 = all
    img = FIX["blocks_160x120"]
    full = fn.fast_detect(img, 10, True)
    k = tie_budget(full[1])
    kxy, kr, _ = fn.fast_detect(img, 10, True, k)
    assert len(kr) > k and kr.min() == np.sort(full[1])[::-1][k - 1]
    keep = full[1] >= kr.min()
    assert np.array_equal(kxy, full[0][keep]) and np.array_equal(kr, full[1][keep])
    # without suppression every response is 0: every key point ties with the cut
    a, b = fn.fast_detect(img, 10, False, 5), fn.fast_detect(img, 10, False, 0)
    assert np.array_equal(a[0], b[0]) and len(a[0]) > 5


# ------------------------------------------------------------------------------------------------------------- fixtures reach their branches
def test_fixtures_are_small():
    for name, img in FIX.items():
        assert img.dtype == np.uint8 and img.shape[0] <= 120 and img.shape[1] <= 160, name


def test_noise_fires_brighter_and_darker_and_has_zero_score_corners():
    g = FIX["noise_64x48"]
    d = fn._ring_minus_centre(g)
    bright, dark = (d > 1)[..., fn.ARCS].all(-1).any(-1), (d < -1)[..., fn.ARCS].all(-1).any(-1)
    assert bright.sum() > 20 and dark.sum() > 20
    f0, s0 = fn.fires(g, 0), fn.score_image(g, 0)
    assert (f0 & (s0 == 0)).any(), "a corner at threshold 0 that scores 0: kept without suppression, never with"
    n_all, n_nms = len(fn.fast_detect(g, 0, False)[0]), len(fn.fast_detect(g, 0, True)[0])
    assert n_all == f0.sum() and 0 < n_nms < n_all


def test_flat_has_no_corner_at_any_threshold():
    for t in (0, 1, 255):
        assert not fn.fires(FIX["flat_40x30"], t).any()


def test_one_corner_7x7_and_the_images_without_an_interior():
    xy, resp, score = fn.fast_detect(FIX["one_corner_7x7"], 10, True)
    assert xy.tolist() == [[3, 3]] and resp.tolist() == [149] and score.sum() == 149
    for name in ("no_interior_20x6", "no_interior_6x20"):
        xy, resp, score = fn.fast_detect(FIX[name], 0, False)
        assert xy.shape == (0, 2) and not score.any()


def test_odd_sizes_have_corners_at_and_past_the_tile_seams():
    # 67 x 35: the last interior column and row (63, 31) read their rings from a tile that holds no interior pixel of its own
    xy, _, _ = fn.fast_detect(FIX["odd_67x35"], 1, False)
    assert xy[:, 0].max() == 63 and xy[:, 1].max() == 31
    # 75 x 41: interior pixels inside the partial tiles on both axes
    xy, _, _ = fn.fast_detect(FIX["partial_tiles_75x41"], 1, False)
    assert (xy[:, 0] >= 64).any() and (xy[:, 1] >= 32).any() and ((xy[:, 0] >= 64) & (xy[:, 1] >= 32)).any()


def test_checkerboard_has_adjacent_tied_scores():
    g = FIX["checkerboard_48x40"]
    f, s = fn.fires(g, 10), fn.score_image(g, 10).astype(int)
    p = np.pad(np.where(f, s, -1), 1, constant_values=-1)
    h, w = s.shape
    tied = np.zeros_like(f)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                tied |= f & (p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w] == s)
    assert tied.sum() > 20 and (f & ~tied).any()                # corners with an equal neighbour, and corners without
    assert 0 < len(fn.fast_detect(g, 10, True)[0]) == (f & ~tied).sum()      # one score everywhere: exactly the untied stay


def test_bgr_fixtures_differ_from_any_single_channel():
    for name in ("bgr_50x37", "bgr_blocks_64x40"):
        img = FIX[name]
        grey = fn.to_gray(img)
        assert all(not np.array_equal(grey, img[..., k]) for k in range(3))
        assert len(fn.fast_detect(img, 1, True)[0]) > 5


def test_blocks_has_many_corners_and_tied_responses():
    xy, resp, _ = fn.fast_detect(FIX["blocks_160x120"], 10, True)
    assert len(xy) > 100 and len(np.unique(resp)) < len(resp)
