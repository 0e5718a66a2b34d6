"""tests/orb_numpy.py -- the blind numpy restatement of the extractor in cv::ORB's shape -- against brute force in its parts,
and against the C oracle (oracle/orb.c: orc_orb_extract_cv) end to end and bit for bit on the images of tests/orb_fixtures.py.
Each fixture also proves, from the restatement's per-level record, that it reaches the branch of the selection it is named
for.  No tolerance anywhere: everything here is integer arithmetic or individually rounded float32."""
import numpy as np
import pytest

import orb_fixtures as fx
import orb_numpy as on

NAMES = ("xy", "octave", "response", "dir", "angle", "desc")


# ---- (a) parts against brute force ------------------------------------------------------------------------------------
def test_run_of_nine_over_all_65536_ring_masks(orc):
    masks = np.arange(1 << 16)
    flags = ((masks[:, None] >> np.arange(16)) & 1).astype(bool)
    by_string = np.array(["1" * 9 in 2 * format(m, "016b") for m in masks])
    assert np.array_equal(on.has_arc9(flags), by_string)
    assert not by_string[0x00FF] and by_string[0x01FF] and by_string[0xF01F] and not by_string[0xF00F] and by_string[0xFFFF]
    # one 7 x 7 patch per mask, 256 x 256 of them in one image: ring pixel k is bright (dark) where bit k is set
    for centre, on_ring, off_ring in ((100, 121, 120), (100, 79, 80), (0, 255, 20), (255, 0, 235)):
        img = np.full((256 * 7, 256 * 7), centre, np.uint8)
        cy, cx = 7 * (masks >> 8) + 3, 7 * (masks & 255) + 3
        for k, (dx, dy) in enumerate(on.RING):
            img[cy + dy, cx + dx] = np.where(flags[:, k], on_ring, off_ring)
        assert np.array_equal(on.fast_fires_at(img, cx, cy, 20), by_string)
        step = 1 if centre == 100 and on_ring == 121 else 7           # every mask once through the C entry, a seventh after
        assert all(orc.fast9(img, cx[m], cy[m], 20) == by_string[m] for m in masks[::step])


def _arc_patches(rng, n):
    """Random 7 x 7 patches whose ring holds an arc of random length at the far side of the centre value, centres 0 and
    255 among them with the ring at (the first sixteenth) or near the opposite extreme."""
    out = []
    for i in range(n):
        c = (0, 255)[i % 2] if i < n // 4 else int(rng.integers(0, 256))
        p = rng.integers(0, 256, (7, 7))
        p[3, 3] = c
        far = 255 - c if i < n // 8 else int(rng.integers(0, 256))
        start, length = int(rng.integers(0, 16)), int(rng.integers(0, 17))
        for j in range(length):
            dx, dy = on.RING[(start + j) % 16]
            p[3 + dy, 3 + dx] = far if i < n // 16 else np.clip(far + rng.integers(-6, 7), 0, 255)
        out.append(p.astype(np.uint8))
    return out


def test_fast_score_is_the_last_threshold_at_which_the_definition_fires(orc):
    """cornerScore = (the smallest threshold at which the segment test no longer fires) - 1, which is the largest at which it
    still does; 0 where that is below the detector's threshold.  Brute force: the definition at every threshold 0..255."""
    rng = np.random.default_rng(17)
    patches = _arc_patches(rng, 1600)
    hit = extreme = 0
    for i, p in enumerate(patches):
        d = np.array([int(p[3 + dy, 3 + dx]) - int(p[3, 3]) for dx, dy in on.RING])
        ts = np.arange(256)[:, None]
        fires = on.has_arc9(d[None, :] > ts) | on.has_arc9(d[None, :] < -ts)
        assert fires[20] == on.fast_fires(p, 20)[3, 3]
        assert not np.any(fires[1:] & ~fires[:-1])                     # monotone: once it stops firing it stays off
        last = int(np.flatnonzero(fires)[-1]) if fires.any() else -1
        for t in (1, 20, (7, 50, 120, 254)[i % 4]):
            want = last if last >= t else 0
            assert orc.fast_score(p, 3, 3, t) == want, (i, t)
            assert on.fast_score_image(p, t)[3, 3] == want, (i, t)
        hit += last >= 20
        extreme += last == 254
    assert hit > 300 and extreme > 20          # the patches do hold corners, and scores at the top of the byte range


@pytest.mark.parametrize("sw,sh,ratio", [(131, 97, 1.2), (97, 131, 1.5), (130, 96, 2.0), (131, 97, 2.0), (203, 77, 2.5), (64, 63, 1.2)])
def test_resize_equals_the_restatement_exactly(orc, sw, sh, ratio):
    rng = np.random.default_rng(sw * 1000 + sh)
    g = rng.integers(0, 256, (sh, sw)).astype(np.uint8)
    dw, dh = int(np.rint(sw / ratio)), int(np.rint(sh / ratio))
    assert np.array_equal(orc.resize_linear(g, dw, dh), on.resize_linear(g, dw, dh))


def test_harris_at_every_pixel_of_a_64x64_image(orc):
    rng = np.random.default_rng(23)
    g = rng.integers(0, 256, (64, 64)).astype(np.uint8)
    g[:, 40:] = np.minimum(g[:, 40:], 30)                              # a strong edge and a dark half among the noise
    ref = on.harris_image(g)
    got = np.array([[orc.harris(g, x, y) for x in range(4, 60)] for y in range(4, 60)], np.float32)
    assert np.array_equal(got, ref[4:60, 4:60])


def test_parts_gauss7_atan2_pattern_levels(orc):
    rng = np.random.default_rng(29)
    g = rng.integers(0, 256, (63, 71)).astype(np.uint8)
    assert list(on.gauss_kernel7()) == [18, 34, 49, 55, 49, 34, 18]
    assert np.array_equal(orc.gauss7(g), on.gauss7(g))
    assert on.umax_from_formula() == on.UMAX_TABLE
    assert len(on.disc_offsets()) == 31 + 2 * (2 * sum(on.UMAX_TABLE[1:]) + 15) == 749      # pixels of the 31-pixel disc
    yx = np.r_[rng.normal(0, 1e5, (500, 2)), [[0, 0], [0, 5], [0, -5], [5, 0], [-5, 0], [3, 3], [-3, 3], [3, -3], [-3, -3]]].astype(np.float32)
    got = np.array([orc.fast_atan2(y, x) for y, x in yx], np.float32)
    assert np.array_equal(got, on.fast_atan2(yx[:, 0], yx[:, 1]))
    assert np.array_equal(on.seeded_pattern(), orc.orb_pattern())
    for (w, h, nl, sf, nf) in [(1241, 376, 8, 1.2, 500), (400, 220, 8, 1.2, 7), (257, 66, 8, 2.5, 300), (63, 63, 4, 2.0, 1)]:
        for a, b in zip(orc.orb_cv_levels(w, h, nl, sf, nf), on.levels_and_quota(w, h, nl, sf, nf)):
            assert np.array_equal(a, b)
    # 7 features over 8 levels: the rounded quotas add up to 8, the last level is left with nothing
    q = on.levels_and_quota(400, 220, 8, 1.2, 7)[3]
    assert list(q) == [2, 1, 1, 1, 1, 1, 1, 0] and q.sum() == 8


# ---- (b) end to end, and what each fixture must reach ----------------------------------------------------------------
_run = fx.reference      # the restatement on one fixture, once per session (tests/test_gpu_orb_edges.py shares it)


def _oracle(orc, img, prm, pat=None):
    return orc.orb_extract_cv(img, prm["n_features"], prm["fast_t"], prm["n_levels"], prm["scale_factor"], pattern=pat)


@pytest.mark.parametrize("random_pattern", [False, True], ids=["seeded", "random15"])
@pytest.mark.parametrize("name", list(fx.cases()))
def test_restatement_equals_oracle_bit_for_bit(orc, name, random_pattern):
    img, prm, pat, res, levels = _run(name, random_pattern)
    o = _oracle(orc, img, prm, pat)
    assert len(o[0]) == len(res[0]) <= prm["n_features"]
    for a, b, what in zip(res, o, NAMES):
        assert a.dtype == b.dtype and np.array_equal(a, b), (name, what)


def test_random_pattern_reaches_the_patch_corner():
    pat = fx.random_pattern()
    assert pat.min() == -15 and pat.max() == 15 and not np.any((pat[:, 0] == pat[:, 2]) & (pat[:, 1] == pat[:, 3]))


def test_motif_takes_both_fallbacks_and_keeps_the_first_in_raster_order():
    img, prm, _, res, levels = _run("motif")
    (l0,) = levels
    print("motif level 0:", {k: v for k, v in l0.items() if k not in ("score", "cand")})
    assert l0["nk"] > 1024 and l0["ties"] > 1024 and l0["ties"] == l0["nk"] and l0["ties_allowed"] == l0["want"] == 200
    assert l0["nc"] > l0["nk"] and l0["fast_cut"] > prm["fast_t"]          # the FAST cut did cut (the motif's second corner)
    sc = l0["score"].ravel()[l0["cand"]]
    assert len(np.unique(sc[sc >= l0["fast_cut"]])) == 1                   # one FAST score among the survivors
    first = l0["cand"][sc >= l0["fast_cut"]][:200]
    assert np.array_equal(res[0], np.stack([first % img.shape[1], first // img.shape[1]], 1).astype(np.float32))


def test_motif_ramp_cuts_inside_a_run_of_equal_responses():
    _, _, _, res, levels = _run("motif_ramp")
    (l0,) = levels
    print("motif_ramp level 0:", {k: v for k, v in l0.items() if k not in ("score", "cand")})
    assert 2 <= l0["ties"] <= 1024 and 0 < l0["ties_allowed"] < l0["ties"]
    assert l0["ties_allowed"] < l0["want"]                                  # some responses lie strictly above the cut
    # the winners among the equals are the raster-earlier ones
    tied = np.flatnonzero(res[2] == np.float32(l0["harris_cut"]))
    assert len(tied) == l0["ties_allowed"]
    idx = (res[0][:, 1] * img_w("motif_ramp") + res[0][:, 0]).astype(np.int64)
    harris = on.harris_image(_run("motif_ramp")[0]).ravel()
    all_tied = np.array([c for c in l0["cand"] if harris[c] == np.float32(l0["harris_cut"]) and l0["score"].ravel()[c] >= l0["fast_cut"]])
    assert len(all_tied) == l0["ties"] and np.array_equal(idx[tied], all_tied[:l0["ties_allowed"]])


def img_w(name):
    return _run(name)[0].shape[1]


def test_sparse_never_cuts():
    _, _, _, res, levels = _run("sparse")
    assert len(levels) == 8 and len(res[0]) > 60
    for L in levels:
        assert 0 < L["nc"] <= 2 * L["want"] and L["nk"] == L["nc"] <= L["want"] and L["harris_cut"] is None and L["n"] == L["nc"]


def test_noise_is_dense_ties_across_tile_borders_and_tops_the_byte_range():
    _, prm, _, res, levels = _run("noise3")
    assert prm["fast_t"] == 1 and len(levels) == 3
    density, meets, top = 0.0, 0, 0
    for L in levels:
        h, w, score = L["h"], L["w"], L["score"].astype(np.int16)
        mask = np.zeros(h * w, bool)
        mask[L["cand"]] = True
        mask = mask.reshape(h, w)
        for y in range(0, h, fx.TILE_H):
            for x in range(0, w, fx.TILE_W):
                density = max(density, mask[y:y + fx.TILE_H, x:x + fx.TILE_W].sum() / (fx.TILE_W * fx.TILE_H / 4))
        assert not np.any(mask[:-1, :] & mask[1:, :]) and not np.any(mask[:, :-1] & mask[:, 1:])      # the 2 x 2 bound's premise
        assert not np.any(mask[:-1, :-1] & mask[1:, 1:]) and not np.any(mask[:-1, 1:] & mask[1:, :-1])
        # a pixel that no neighbour beats and that an equal neighbour on the other side of a tile border ties: strict
        # suppression drops both, a non-strict comparison on either side would keep one
        pad = np.pad(score, 1)
        nb_max = np.max([pad[1 + dy:1 + dy + h, 1 + dx:1 + dx + w] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dx or dy], axis=0)
        peak = (score > 0) & (score >= nb_max)
        inside = np.zeros((h, w), bool)
        inside[on.EDGE:h - on.EDGE, on.EDGE:w - on.EDGE] = True
        peak &= inside
        for x in range(fx.TILE_W, w, fx.TILE_W):
            meets += int(np.sum(peak[:, x - 1] & peak[:, x] & (score[:, x - 1] == score[:, x])))
        for y in range(fx.TILE_H, h, fx.TILE_H):
            meets += int(np.sum(peak[y - 1, :] & peak[y, :] & (score[y - 1, :] == score[y, :])))
        top = max(top, int(L["score"].ravel()[L["cand"]].max()))
    print(f"noise3: densest tile {density:.3f} of the one-per-2x2 bound, {meets} equal peaks across tile borders, top score {top}")
    assert density > 0.25 and meets >= 1 and top >= 250
    assert any(L["nc"] > 2 * L["want"] and L["nk"] > L["want"] for L in levels)


@pytest.mark.parametrize("name", [n for n in fx.cases() if n.startswith("geom_")])
def test_geometry_levels_switch_off_and_still_find_the_lone_corner(name):
    img, prm, _, res, levels = _run(name)
    h, w = img.shape
    ws, hs, _, _ = on.levels_and_quota(w, h, prm["n_levels"], prm["scale_factor"], prm["n_features"])
    assert len(levels) < prm["n_levels"] and (ws[len(levels)] <= 62 or hs[len(levels)] <= 62)      # upper levels are off
    if prm["scale_factor"] == 2.5:
        assert ws[-1] < 8 and hs[-1] < 8                                                                # and truncated
    assert np.any(np.all(res[0] == np.float32(31), axis=1) & (res[1] == 0))                             # the pixel at (31, 31)
    assert levels[0]["n"] >= 1


@pytest.mark.parametrize("nf", [1, 7, 8])
def test_small_budgets_stay_within_the_budget(nf):
    _, prm, _, res, levels = _run(f"budget_{nf}")
    assert prm["n_levels"] == 8 and len(res[0]) <= nf
    assert sum(L["n"] for L in levels) == len(res[0])
    if nf == 7:      # quotas 2 1 1 1 1 1 1 (+ 0) add up to 8: the seventh level runs out of budget
        assert [L["quota"] for L in levels] == [2, 1, 1, 1, 1, 1, 1] and levels[-1]["want"] == 0 and len(res[0]) == 7
    if nf == 8:
        assert len(res[0]) == 8 and [L["n"] for L in levels] == [2, 1, 1, 1, 1, 1, 1]
