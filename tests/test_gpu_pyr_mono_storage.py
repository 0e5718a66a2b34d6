"""Grey frames given as BGR are stored in one channel (pyramid.hip: the head launch decides per pyramid and build; lk.hip: the
one-channel body stages one-channel tiles from the grey regions, lk_expand_kernel fills the three-channel regions for the
pairs that need them).  Nothing may change: the read-backs return the three-channel bytes and words of tests/pyr_numpy.py's
definition, the tracker's outputs equal the THREE-channel oracle bit for bit, and all of it equals the same calls under
SVO_PYR_MONO_STORAGE=0.  The switches are read once per process, so every setting runs `_child` in a fresh process (this file,
run as a script) and the tests compare what the children saved.  The storage word has no accessor in the C ABI: `_stored_word`
reads it out of the pyramid's device header (svo_internal.h: `base` is the member behind the four ints of svo_pyramid, the
words sit at its first bytes), so that a build which never stored grey cannot pass.

Shapes: the three-channel entries of tests/pyr_fixtures.py's seam table (narrow, short, tile seams, 1 to 4 levels) for the
levels; 160 x 120 x 3 for the tracker; 192 x 96 x 3 over 12 frames for the front-end (one chunk, and a lock-step group of four
chunks that start one frame apart)."""
import ctypes
import os
import pathlib
import subprocess
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import pyr_fixtures as pf  # noqa: E402

pytestmark = pytest.mark.gpu

W, H = 160, 120
ENTRIES = [e for e in pf.TABLE if e.c == 3]
SETTINGS = {"default": {}, "storage0": {"SVO_PYR_MONO_STORAGE": "0"}, "mono0": {"SVO_LK_MONO": "0"},
            "storage0_mono0": {"SVO_PYR_MONO_STORAGE": "0", "SVO_LK_MONO": "0"}}


def _grey_image(e, seed=0):
    return pf.grey(pf.image(e.w, e.h, 3, "ramps", seed))


def _pair(colour=False, seed=5, shift=(1.3, -0.7)):
    from ros_stereo_slam_amd import synth

    if colour:
        return synth.textured_pair(W, H, 3, shift=shift, seed=seed, colour=True)
    a, b = synth.textured_pair(W, H, 1, shift=shift, seed=seed)
    a, b = a.reshape(H, W, 1), b.reshape(H, W, 1)
    return np.ascontiguousarray(np.repeat(a, 3, 2)), np.ascontiguousarray(np.repeat(b, 3, 2))


def _points():
    """About 300: the lattice, fractional points, points within a window of every border, the corners, points outside."""
    rng = np.random.default_rng(23)
    gx, gy = np.meshgrid(np.arange(8, W - 7, 8, dtype=np.float32), np.arange(8, H - 7, 8, dtype=np.float32))
    lat = np.stack([gx.ravel(), gy.ravel()], 1)
    frac = rng.uniform([12, 12], [W - 12, H - 12], (60, 2)).astype(np.float32)
    edge = rng.uniform([-6, -6], [W + 6, H + 6], (40, 2)).astype(np.float32)
    corners = np.array([[0, 0], [W - 1, 0], [0, H - 1], [W - 1, H - 1], [0.5, 0.5], [W - 1.5, H - 1.5]], np.float32)
    return np.concatenate([lat, frac, edge, corners])


def _bits(o, st, err, me):
    return np.concatenate([np.ascontiguousarray(o, np.float32).view(np.uint32).ravel(), np.asarray(st, np.uint32).ravel(),
                           np.ascontiguousarray(err, np.float32).view(np.uint32).ravel(),
                           np.ascontiguousarray(me, np.float32).view(np.uint32).ravel()])


def _readbacks(p):
    out = []
    for l in range(p.levels):
        out += [p.level(l).ravel(), p.padded_level(l).ravel(), p.derivative_level(l).view(np.uint8).ravel()]
    return np.concatenate(out)


def _off_grey(img, where):
    """One byte off grey: the first pixel, the last byte of the last row, and the bytes on either side of a dword seam."""
    out = img.copy()
    flat = out.reshape(-1)
    i = {"first": 0, "last": flat.size - 1, "seam_lo": 4 * (flat.size // 8) - 1, "seam_hi": 4 * (flat.size // 8)}[where]
    flat[i] = flat[i] + 1 if flat[i] < 255 else 254
    return out


WHERE = ("first", "last", "seam_lo", "seam_hi")
SVO_PYR_STORED = 2  # svo_internal.h


def _stored_word(ctx, p):
    """SVO_PYR_STORED of a pyramid: 1 = the last build stored grey, 3 = three channels, 0 = never built."""
    base = ctypes.c_void_p.from_address(p._h.value + 16).value  # struct svo_pyramid { int w, h, c, levels; uint8_t *base; ..
    word = ctypes.c_int(-1)
    ctx.sync()
    hip_memcpy = ctx.lib.hipMemcpy  # the HIP runtime the library is linked against
    hip_memcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    assert hip_memcpy(ctypes.byref(word), ctypes.c_void_p(base + 4 * SVO_PYR_STORED), 4, 2) == 0  # 2: device to host
    return np.array(word.value)


GROUP = 4  # chunks of the lock-step group; chunk k takes frames k .. k + 11 of a stream of 15


def _stream(n=12, colour_at=None, colour_right_at=None):
    from ros_stereo_slam_amd import synth

    size, K4 = (192, 96), (150.0, 150.0, 96.0, 48.0)
    scene = synth.Scene()
    lefts, rights = [], []
    for i, (R, t) in enumerate(synth.corridor_trajectory(n, step=0.3)):
        l, r = scene.stereo(R, t, K=K4, size=size)[:2]
        l, r = (np.ascontiguousarray(np.repeat(x.reshape(size[1], size[0], -1)[..., :1], 3, 2)) for x in (l, r))
        if i == colour_at:
            l = l.copy()
            l[..., 1] = 255 - l[..., 1]
        if i == colour_right_at:
            r = r.copy()
            r[..., 2] = r[..., 2] // 2
        lefts.append(l)
        rights.append(r)
    return size, K4, lefts, rights


def _child(out):
    import torch

    torch.cuda.is_available()
    from ros_stereo_slam_amd import capi

    ctx = capi.Context(0)
    res = {}
    # ---- levels: the seam table, grey; then one pyramid object grey -> colour -> grey; one byte off grey
    for e in ENTRIES:
        p = ctx.pyramid(e.w, e.h, 3, e.levels)
        g, col = _grey_image(e), pf.image(e.w, e.h, 3, "ramps")
        for k, img in enumerate((g, col, _grey_image(e, 1))):
            p.build(np.ascontiguousarray(img))
            res[f"lv_{pf.entry_id(e)}_{k}"] = _readbacks(p)
            res[f"mono_{pf.entry_id(e)}_{k}"] = np.array(p.is_mono())
            res[f"stored_{pf.entry_id(e)}_{k}"] = _stored_word(ctx, p)
        p.close()
    e = ENTRIES[0]
    p = ctx.pyramid(e.w, e.h, 3, e.levels)
    for wh in WHERE:
        p.build(_off_grey(_grey_image(e), wh))
        res[f"off_{wh}"] = _readbacks(p)
        res[f"offmono_{wh}"] = np.array(p.is_mono())
        res[f"stored_off_{wh}"] = _stored_word(ctx, p)
    # a gated-off build leaves the words and both regions alone: grey-stored, then colour-stored
    shut = torch.zeros(1, dtype=torch.int32, device="cuda")
    g, col = np.ascontiguousarray(_grey_image(e)), np.ascontiguousarray(pf.image(e.w, e.h, 3, "ramps"))
    dg, dc = torch.from_numpy(g).cuda(), torch.from_numpy(col).cuda()
    p.build(g)
    p.build_gated(dc, shut)
    res["stored_gated_grey"] = _stored_word(ctx, p)
    res["gated_grey"], res["gated_grey_mono"] = _readbacks(p), np.array(p.is_mono())
    p.build(col)
    p.build_gated(dg, shut)
    res["stored_gated_colour"] = _stored_word(ctx, p)
    res["gated_colour"], res["gated_colour_mono"] = _readbacks(p), np.array(p.is_mono())
    p.close()
    # 32 jobs of one set: grey and colour mixed, every fifth gated off (it keeps the other kind from a build before)
    pyrs = [ctx.pyramid(e.w, e.h, 3, e.levels) for _ in range(32)]
    for k, q in enumerate(pyrs):
        q.build(col if k % 2 else g)
    imgs = [dg if k % 3 else dc for k in range(32)]
    gates = [shut if k % 5 == 4 else None for k in range(32)]
    ctx.build_pyramids(pyrs, imgs, gates)
    ctx.sync()
    for k, q in enumerate(pyrs):
        res[f"stored_many_{k}"] = _stored_word(ctx, q)
        res[f"many_{k}"], res[f"manymono_{k}"] = _readbacks(q), np.array(q.is_mono())
        q.close()

    # ---- tracker
    pts = _points()
    ga, gb = _pair()
    ca, cb = _pair(colour=True)
    ga2, gb2 = _pair(seed=8, shift=(-0.8, 1.1))
    mk = lambda img, **kw: ctx.pyramid(W, H, 3, **kw).build(img)  # noqa: E731
    pga, pgb, pca, pcb = mk(ga), mk(gb), mk(ca), mk(cb)
    res["t_gg"] = _bits(*ctx.lk_track(pga, pgb, pts))
    res["t_gc"] = _bits(*ctx.lk_track(pga, pcb, pts))   # expands pga
    res["t_cg"] = _bits(*ctx.lk_track(pca, pgb, pts))   # expands pgb
    res["t_gg_again"] = _bits(*ctx.lk_track(pga, pgb, pts))
    pgb.build(gb2)                                       # the rebuild clears the mark
    res["t_gg2"] = _bits(*ctx.lk_track(pga, pgb, pts))
    res["t_cg2"] = _bits(*ctx.lk_track(pca, pgb, pts))
    pgb.build(gb)
    # a first image created without derivative levels, grey/grey and grey/colour
    pnd = mk(ga, want_deriv=False)
    res["t_nd_gg"] = _bits(*ctx.lk_track(pnd, pgb, pts))
    pnd.build(ga)
    res["t_nd_gc"] = _bits(*ctx.lk_track(pnd, pcb, pts))
    # a gated-off colour build into a grey-stored pyramid whose three-channel regions are expanded and valid: the next
    # track reads those regions as they are (no new expansion), so a byte the gated build wrote there shows
    pgate = mk(ga)
    res["t_gate_before"] = _bits(*ctx.lk_track(pgate, pcb, pts))
    pgate.build_gated(torch.from_numpy(ca).cuda(), torch.zeros(1, dtype=torch.int32, device="cuda"))
    res["t_gate_after"] = _bits(*ctx.lk_track(pgate, pcb, pts))
    res["t_gate_second"] = _bits(*ctx.lk_track(pcb, pgate, pts))
    # 16 jobs of one launch, all four kinds of pair, against their own launches
    pairs = [(pga, pgb), (pca, pcb), (mk(ga), pcb), (pca, mk(gb)), (mk(ga2), mk(gb2)), (pgb, pga), (pcb, pca), (mk(gb2), mk(ga2))] * 2
    n = len(pts)
    dp = torch.from_numpy(pts).cuda()
    outs = [(torch.zeros(n, 2, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda"), torch.zeros(n, device="cuda"),
             torch.zeros(n, device="cuda")) for _ in pairs]
    ctx.lk_track_jobs([(a, b, dp, o[0], o[1], o[2], o[3], None) for (a, b), o in zip(pairs, outs)])
    ctx.sync()
    for k, ((a, b), o) in enumerate(zip(pairs, outs)):
        res[f"jobs_{k}"] = _bits(*[t.cpu().numpy() for t in o])
        res[f"jobs_own_{k}"] = _bits(*ctx.lk_track(a, b, pts))
    # ---- colours
    xy = np.concatenate([pts, [[-3.0, 2.0], [W + 5.0, H + 5.0]]]).astype(np.float32)
    res["colours_grey"] = np.asarray(ctx.get_colors(mk(ga), xy), np.float32).view(np.uint32).ravel()
    res["colours_colour"] = np.asarray(ctx.get_colors(pca, xy), np.float32).view(np.uint32).ravel()
    # ---- front-end: a chunk of 12 frames, and a lock-step group of four chunks that start one frame apart: all grey; a
    # colour left frame in the middle; a colour right image at a frame that the grey run made a keyframe
    def front_end(name, **kw):
        size, K4, lefts, rights = _stream(n=12 + GROUP - 1, **kw)
        vo = capi.VisualOdometry(ctx, size[0], size[1], 3, grid_step=12, keyframe_min_inliers=90, seed=7, K4=K4)
        vo.init(lefts[0], rights[0])
        r = vo.run_chunk(lefts[1:12], rights[1:12])
        res[f"vo_{name}"] = np.concatenate([np.ascontiguousarray(np.asarray(x, np.float64)).view(np.uint8).ravel() for x in r])
        res[f"vo_{name}_kf"] = np.asarray(r[-1])
        vo.close()
        vos = [capi.VisualOdometry(ctx, size[0], size[1], 3, grid_step=12, keyframe_min_inliers=90, seed=7 + k, K4=K4)
               for k in range(GROUP)]
        rs = capi.run_chunks([(v, lefts[k:k + 12], rights[k:k + 12]) for k, v in enumerate(vos)], init=True)
        for k, r in enumerate(rs):
            res[f"vo4_{name}_{k}"] = np.concatenate([np.ascontiguousarray(np.asarray(x, np.float64)).view(np.uint8).ravel() for x in r])
            res[f"vo4_{name}_{k}_kf"] = np.asarray(r[-1])
        for v in vos:
            v.close()

    front_end("grey")
    front_end("colour_mid", colour_at=6)
    # entry i of a chunk's keyframe array is the chunk's frame i + 1; chunk 0 and the single chunk start at stream frame 0
    kf = np.flatnonzero(res["vo_grey_kf"])
    at = int(kf[0]) + 1 if len(kf) else 4
    res["colour_right_at"] = np.array(at)
    front_end("colour_right", colour_right_at=at)
    np.savez(out, **res)
    ctx.close()


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("mono_storage")
    out = {}
    for name, env in SETTINGS.items():
        f = d / f"{name}.npz"
        r = subprocess.run([sys.executable, __file__, str(f)], env=dict(os.environ, **env), capture_output=True, text=True,
                           timeout=600, cwd=str(ROOT))
        assert r.returncode == 0, name + ": " + r.stdout[-2000:] + r.stderr[-4000:]
        out[name] = dict(np.load(f))
    return out


def _definition_bytes(img, levels):
    d = pf.define(np.ascontiguousarray(img), levels)
    out = []
    for l in range(levels):
        out += [d.levels[l].ravel(), d.padded[l].ravel(), np.ascontiguousarray(d.words[l]).view(np.uint8).ravel()]
    return np.concatenate(out)


def test_every_setting_gives_the_storage_off_bytes(runs):
    """Every array of every child -- read-backs, words, tracks, colours, front-end records -- bit for bit."""
    ref = runs["storage0"]
    for name, got in runs.items():
        assert sorted(got) == sorted(ref)
        for k in ref:
            if k.startswith("stored_"):
                continue  # the one thing that differs: test_the_storage_word_follows_every_build
            assert np.array_equal(got[k], ref[k]), f"{name}: {k} differs from SVO_PYR_MONO_STORAGE=0"


@pytest.mark.parametrize("e", ENTRIES, ids=pf.entry_id)
def test_levels_of_grey_colour_grey_builds_equal_the_definition(runs, e):
    got = runs["default"]
    for k, (img, mono) in enumerate(((_grey_image(e), True), (pf.image(e.w, e.h, 3, "ramps"), False), (_grey_image(e, 1), True))):
        assert np.array_equal(got[f"lv_{pf.entry_id(e)}_{k}"], _definition_bytes(img, e.levels)), f"build {k}"
        # a one-level pyramid with derivative levels still has a finishing launch, so it reports its word too
        assert bool(got[f"mono_{pf.entry_id(e)}_{k}"]) == mono


@pytest.mark.parametrize("where", WHERE)
def test_one_byte_off_grey_gives_colour_storage(runs, where):
    e = ENTRIES[0]
    img = _off_grey(_grey_image(e), where)
    assert not (img[..., 0] == img[..., 1]).all() or not (img[..., 1] == img[..., 2]).all()
    assert np.array_equal(runs["default"][f"off_{where}"], _definition_bytes(img, e.levels))
    assert not bool(runs["default"][f"offmono_{where}"])


def test_a_gated_build_leaves_words_and_regions_alone(runs):
    e, got = ENTRIES[0], runs["default"]
    assert np.array_equal(got["gated_grey"], _definition_bytes(_grey_image(e), e.levels)) and bool(got["gated_grey_mono"])
    assert np.array_equal(got["gated_colour"], _definition_bytes(pf.image(e.w, e.h, 3, "ramps"), e.levels))
    assert not bool(got["gated_colour_mono"])


def test_the_storage_word_follows_every_build(runs):
    """Grey images are stored grey (1) unless SVO_PYR_MONO_STORAGE=0 (3), colour images never; the tracker's switch does not
    matter; a gated-off build leaves the word."""
    for name, got in runs.items():
        g = 3 if "storage0" in name else 1
        for e in ENTRIES:
            assert [int(got[f"stored_{pf.entry_id(e)}_{k}"]) for k in range(3)] == [g, 3, g], f"{name}: {pf.entry_id(e)}"
        assert [int(got[f"stored_off_{wh}"]) for wh in WHERE] == [3] * len(WHERE), name
        assert (int(got["stored_gated_grey"]), int(got["stored_gated_colour"])) == (g, 3), name
        for k in range(32):
            grey = (k % 2 == 0) if k % 5 == 4 else (k % 3 != 0)
            assert int(got[f"stored_many_{k}"]) == (g if grey else 3), f"{name}: job {k} of the set"


def test_thirty_two_mixed_jobs_of_one_set(runs):
    e, got = ENTRIES[0], runs["default"]
    g, col = _definition_bytes(_grey_image(e), e.levels), _definition_bytes(pf.image(e.w, e.h, 3, "ramps"), e.levels)
    for k in range(32):
        grey = (k % 2 == 0) if k % 5 == 4 else (k % 3 != 0)
        assert np.array_equal(got[f"many_{k}"], g if grey else col), f"job {k}"
        assert bool(got[f"manymono_{k}"]) == grey, f"job {k}"


def test_tracks_equal_the_three_channel_oracle(runs, orc):
    pts = _points()
    ga, gb = _pair()
    ca, cb = _pair(colour=True)
    _, gb2 = _pair(seed=8, shift=(-0.8, 1.1))
    want = {"t_gg": (ga, gb), "t_gc": (ga, cb), "t_cg": (ca, gb), "t_gg_again": (ga, gb), "t_gg2": (ga, gb2), "t_cg2": (ca, gb2),
            "t_nd_gg": (ga, gb), "t_nd_gc": (ga, cb)}
    for name, got in runs.items():
        for k, (a, b) in want.items():
            assert np.array_equal(got[k], _bits(*orc.lk_track(a, b, pts))), f"{name}: {k}"
    assert _bits(*orc.lk_track(ga, gb, pts))[2 * len(pts):3 * len(pts)].mean() >= 0.6, "the oracle should track most points"


def test_a_gated_build_does_not_touch_expanded_three_channel_regions(runs, orc):
    pts = _points()
    ga, _ = _pair()
    _, cb = _pair(colour=True)
    for name, got in runs.items():
        want = _bits(*orc.lk_track(ga, cb, pts))
        assert np.array_equal(got["t_gate_before"], want) and np.array_equal(got["t_gate_after"], want), name
        assert np.array_equal(got["t_gate_second"], _bits(*orc.lk_track(cb, ga, pts))), name


def test_sixteen_jobs_equal_their_own_launches(runs):
    for name, got in runs.items():
        for k in range(16):
            assert np.array_equal(got[f"jobs_{k}"], got[f"jobs_own_{k}"]), f"{name}: job {k}"


def test_keyframes_fire_where_the_front_end_runs_need_them(runs):
    got = runs["default"]
    for name in ("grey", "colour_mid", "colour_right"):
        assert np.asarray(got[f"vo_{name}_kf"]).any(), f"{name}: choose grid_step so that a keyframe fires"
        assert any(np.asarray(got[f"vo4_{name}_{k}_kf"]).any() for k in range(GROUP)), f"{name}: no keyframe in the group"
    # the colour right image sits at a keyframe: of the single chunk and of chunk 0 of the group (stream frame `at`), and it
    # is frame at - k of chunk k
    at = int(got["colour_right_at"])
    assert got["vo_colour_right_kf"][at - 1] and got["vo_grey_kf"][at - 1]
    assert any(at - k >= 1 and got[f"vo4_colour_right_{k}_kf"][at - k - 1] for k in range(GROUP)), "no chunk of the group has it at a keyframe"


if __name__ == "__main__":
    _child(sys.argv[1])
