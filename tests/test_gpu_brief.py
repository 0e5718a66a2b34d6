"""svo_brief_* against the numpy restatement (tests/brief_numpy.py) fed with the library's own test table, bit for bit: both
sides are integer arithmetic behind two stated roundings, so the bar is np.array_equal on the integral image, the descriptor rows and
kept_index.

End to end: on a rendered stereo pair SIFT key points -> brief_describe -> knn_match -> ratio_pairs equals the CPU composition
(brief_numpy on the same key points, match_numpy) pair for pair, and the C++ adaptor with BRIEF_FLAG = true reproduces the pairs, the
F-inliers and the triangulated points of the Python path."""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest

import brief_numpy as bn
import match_numpy as mn
from ros_stereo_slam_amd import capi, sequence, synth

pytestmark = pytest.mark.gpu

K4_SMALL = (360.0, 360.0, 320.0, 120.0)
COUNTS = (0, 1, 63, 64, 65, 20000)     # the wave-boundary counts and the reference's SIFT budget


@functools.lru_cache(maxsize=None)
def image(key):
    """57x57 and 65x60: noise (a single admissible pixel / two strips of the row scan's wave); the two frame sizes: the rendered scene"""
    rng = np.random.default_rng(5)
    if key == "57x57":
        return rng.integers(0, 256, (57, 57), dtype=np.uint8)
    if key == "65x60":
        return rng.integers(0, 256, (60, 65), dtype=np.uint8)
    R, t = synth.corridor_trajectory(1, step=0.5)[0]
    if key == "640x240":
        return np.ascontiguousarray(synth.Scene().render(R, t, K=K4_SMALL, size=(640, 240), channels=3)[0])
    assert key == "1241x376"
    return np.ascontiguousarray(synth.Scene().render(R, t, channels=1)[0].reshape(376, 1241))


IMAGES = ("57x57", "65x60", "640x240", "1241x376")


def planted(w, h):
    """the half-integer and border cases of tests/test_brief_numpy.py"""
    lo = np.nextafter(np.float32(27.5), np.float32(0))
    xs = [27.5, 28.5, float(lo), 27.49, 28.0, w - 29.0, w - 28.0, w - 28.5, w - 29.5, 40.5, float(np.nextafter(np.float32(40.5), np.float32(0)))]
    ys = [27.5, 28.5, float(lo), 27.49, 28.0, h - 29.0, h - 28.0, h - 28.5, h - 29.5]
    pts = [(x, 28.0) for x in xs] + [(28.0, y) for y in ys] + [(x, h - 29.0) for x in xs] + [(w - 29.0, y) for y in ys]
    pts += [(np.nan, 30.0), (30.0, np.nan), (np.inf, 30.0), (30.0, -np.inf), (1e30, 30.0), (-1e30, -1e30)]
    return np.array(pts, np.float32)


@functools.lru_cache(maxsize=None)
def keypoints(key, n, seed=0):
    img = image(key)
    h, w = img.shape[:2]
    rng = np.random.default_rng([seed, w, h, n])
    if n == 1:
        return np.array([[28.25, 27.75]], np.float32)
    xy = rng.uniform([-40, -40], [w + 40, h + 40], (n, 2))
    near = rng.random(n) < 0.4     # a share inside or just outside the admissible rectangle, so that small images keep some
    xy[near] = rng.uniform([26, 26], [w - 26, h - 26], (int(near.sum()), 2))
    xy = xy.astype(np.float32)
    p = planted(w, h)
    if n >= len(p):
        xy[rng.choice(n, len(p), replace=False)] = p
    return xy


@functools.lru_cache(maxsize=None)
def restated(key, nbytes, n, seed=0):
    return bn.describe(image(key), keypoints(key, n, seed), capi.brief_default_pattern(nbytes), nbytes)


def assert_same(got, ref, what):
    assert got[1].dtype == np.int32 and got[0].dtype == np.uint8
    assert np.array_equal(got[1], ref[1]), f"{what}: kept_index differs ({len(got[1])} kept, the restatement keeps {len(ref[1])})"
    bad = np.flatnonzero((got[0] != ref[0]).any(1)) if len(ref[0]) else []
    assert got[0].shape == ref[0].shape and len(bad) == 0, f"{what}: {len(bad)} descriptors differ, first row {bad[0] if len(bad) else '-'}"


# ---- the integral image ----
@pytest.mark.parametrize("key", IMAGES)
def test_integral_equals_the_restatement(ctx, key):
    img = image(key)
    got = ctx.brief_integral(img)
    assert got.dtype == np.int32 and np.array_equal(got, bn.integral(bn.to_grey(img)))


def test_integral_of_the_largest_sum(ctx):
    got = ctx.brief_integral(np.full((376, 1241), 255, np.uint8))
    y, x = np.mgrid[0:377, 0:1242]
    assert np.array_equal(got, 255 * y * x) and int(got[-1, -1]) == 255 * 376 * 1241


# ---- descriptors ----
@pytest.mark.parametrize("nbytes", [16, 32, 64])
@pytest.mark.parametrize("key", IMAGES)
def test_descriptors_equal_the_restatement(ctx, key, nbytes):
    """one call per (image, length): a batch of six copies of the image, one per key-point count"""
    img = image(key)
    got = ctx.brief_describe([img] * len(COUNTS), [keypoints(key, n) for n in COUNTS], nbytes)
    kept = []
    for n, g in zip(COUNTS, got):
        ref = restated(key, nbytes, n)
        assert_same(g, ref, f"{key}, {nbytes} bytes, {n} key points")
        kept.append(len(ref[1]))
    print(f"{key} {nbytes} bytes: kept {kept} of {list(COUNTS)}")
    assert kept[0] == 0 and kept[1] == 1 and kept[-1] >= 1
    assert min(kept[2:]) >= (10 if key in ("640x240", "1241x376") else 1)


def test_a_set_table_and_back_to_the_default(ctx):
    key, n = "640x240", 3000
    img, xy = image(key), keypoints(key, 3000)
    before = ctx.brief_describe([img], [xy], 32)[0]
    assert_same(before, restated(key, 32, n), "default table")
    rng = np.random.default_rng(8)
    table = rng.integers(-24, 25, (256, 4)).astype(np.int8)
    table[:4] = [(-24, -24, 24, 24), (24, -24, -24, 24), (24, 24, -24, -24), (-24, 24, 24, -24)]    # all four corners of the patch
    same = (table[:, 0] == table[:, 2]) & (table[:, 1] == table[:, 3])
    table[same, 2] = -table[same, 2] + (table[same, 2] == 0)
    try:
        ctx.brief_set_pattern(table, 32)
        assert_same(ctx.brief_describe([img], [xy], 32)[0], bn.describe(img, xy, table, 32), "set table")
        assert_same(ctx.brief_describe([img], [xy], 64)[0], restated(key, 64, n), "the 64-byte table is untouched")
        for bad in (np.where(np.arange(1024).reshape(256, 4) == 517, 25, table), np.where(np.arange(1024).reshape(256, 4) == 3, -25, table),
                    np.concatenate([table[:100], [[3, 4, 3, 4]], table[101:]])):
            with pytest.raises(capi.SvoError) as e:
                ctx.brief_set_pattern(bad, 32)
            assert e.value.code == capi.SVO_ERR_ARG
        assert_same(ctx.brief_describe([img], [xy], 32)[0], bn.describe(img, xy, table, 32), "a refused table changes nothing")
    finally:
        ctx.brief_set_pattern(None, 32)
    after = ctx.brief_describe([img], [xy], 32)[0]
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])


# ---- batches and memory ----
def batch_inputs(nimg):
    base = image("640x240")
    imgs = [np.ascontiguousarray(np.roll(base, 37 * k, axis=1)) for k in range(nimg)]
    pts = [keypoints("640x240", 500 + 61 * k, seed=k + 1) for k in range(nimg)]
    return imgs, pts


@pytest.mark.parametrize("nimg", [2, 16])
def test_batch_equals_one_call_per_image(ctx, nimg):
    imgs, pts = batch_inputs(nimg)
    batch = ctx.brief_describe(imgs, pts, 32)
    table = capi.brief_default_pattern(32)
    for k in range(nimg):
        single = ctx.brief_describe([imgs[k]], [pts[k]], 32)[0]
        assert len(single[1]) >= 100
        assert np.array_equal(batch[k][0], single[0]) and np.array_equal(batch[k][1], single[1]), f"image {k} of a batch of {nimg}"
    assert_same(batch[nimg - 1], bn.describe(imgs[nimg - 1], pts[nimg - 1], table, 32), "last image of the batch")


def test_device_memory_equals_host_memory(ctx):
    import torch

    imgs, pts = batch_inputs(3)
    for nbytes in (16, 64):
        host = ctx.brief_describe(imgs, pts, nbytes)
        dev = ctx.brief_describe([torch.from_numpy(im).cuda() for im in imgs], [torch.from_numpy(p).cuda() for p in pts], nbytes)
        for h_, d_ in zip(host, dev):
            assert len(h_[1]) >= 100 and np.array_equal(h_[0], d_[0]) and np.array_equal(h_[1], d_[1])


# ---- refusals ----
def raw_call(ctx, img, xy, n_in, cap, kept, desc, n_out, w=None, h=None, c=None, nbytes=32, nimg=1, images=True, mem=capi.MEM_HOST):
    ih, iw = img.shape[:2]
    ptrs = (C.c_void_p * 16)(*([img.ctypes.data] * 16))
    nin = (C.c_int * 16)(*([n_in] * 16)) if n_in is not None else None
    return ctx.lib.svo_brief_describe_batch(ctx._h, ptrs if images else None, nimg, iw if w is None else w, ih if h is None else h,
                                            (1 if img.ndim == 2 else img.shape[2]) if c is None else c, nbytes, xy, nin, cap, kept, desc,
                                            n_out, mem)


def test_refusals_leave_the_outputs_untouched(ctx):
    img = image("640x240")
    cap = 64
    xy = np.ascontiguousarray(keypoints("640x240", 64))
    kept, desc, n_out = np.full(cap + 1, -7, np.int32), np.full(cap * 64 + 8, 0xA5, np.uint8), np.full(16, -9, np.int32)
    p = lambda a, off=0: C.c_void_p(a.ctypes.data + off)   # noqa: E731
    good = dict(xy=p(xy), n_in=64, cap=cap, kept=p(kept), desc=p(desc), n_out=p(n_out))

    def refused(code=capi.SVO_ERR_ARG, **kw):
        a = dict(good, **{k: v for k, v in kw.items() if k in good})
        rest = {k: v for k, v in kw.items() if k not in good}
        rc = raw_call(ctx, img, a["xy"], a["n_in"], a["cap"], a["kept"], a["desc"], a["n_out"], **rest)
        assert rc == code, (kw, rc)
        assert np.all(kept == -7) and np.all(desc == 0xA5) and np.all(n_out == -9), kw

    refused(xy=None)
    refused(n_in=None)
    refused(kept=None)
    refused(desc=None)
    refused(n_out=None)
    refused(images=False)
    refused(xy=p(xy, 2))
    refused(kept=p(kept, 1))
    refused(n_out=p(n_out, 2))
    refused(c=2)
    refused(c=4)
    for nb in (0, 8, 24, 33, 128):
        refused(nbytes=nb)
    refused(nimg=0)
    refused(nimg=17)
    refused(cap=0)
    refused(n_in=-1)
    refused(n_in=cap + 1)
    refused(w=0)
    refused(h=0)
    refused(w=16385)
    refused(h=16385)
    refused(mem=2)
    # 255 * 16384 * 16384 > 2^31 - 1: decided before the 256 MB image is looked at (the pointer only holds a small one)
    refused(code=capi.SVO_ERR_CAPACITY, w=16384, h=16384)
    refused(code=capi.SVO_ERR_CAPACITY, w=2901, h=2903)                 # 255 * 8421603 = 2^31 + 25117
    big = np.zeros(4, np.int32)
    assert ctx.lib.svo_brief_integral(ctx._h, p(img), 16384, 16384, 1, p(big), capi.MEM_HOST) == capi.SVO_ERR_CAPACITY and not big.any()
    assert ctx.lib.svo_brief_integral(ctx._h, p(img), 640, 240, 2, p(big), capi.MEM_HOST) == capi.SVO_ERR_ARG
    assert ctx.lib.svo_brief_integral(ctx._h, p(img), 640, 240, 3, p(big, 1), capi.MEM_HOST) == capi.SVO_ERR_ARG
    # the same arguments, accepted
    assert raw_call(ctx, img, good["xy"], 64, cap, good["kept"], good["desc"], good["n_out"]) == 0
    ref = restated("640x240", 32, 64)
    assert n_out[0] == len(ref[1]) and n_out[1] == -9 and np.array_equal(kept[:n_out[0]], ref[1]) and kept[cap] == -7
    assert np.array_equal(desc[:32 * n_out[0]].reshape(-1, 32), ref[0]) and np.all(desc[32 * cap:] == 0xA5)


def test_an_image_below_the_border_keeps_nothing(ctx):
    tiny = np.random.default_rng(6).integers(0, 256, (40, 40), dtype=np.uint8)
    pts = np.random.default_rng(7).uniform(0, 40, (100, 2)).astype(np.float32)
    for im in (tiny, np.zeros((56, 300), np.uint8), np.zeros((300, 56, 3), np.uint8)):
        desc, kept = ctx.brief_describe([im], [pts], 32)[0]
        assert desc.shape == (0, 32) and kept.shape == (0,)
        assert np.array_equal(ctx.brief_integral(im), bn.integral(bn.to_grey(im)))


# ---- the chain of StereoProcess::stereoTriangulate ----
N_FEATURES = 2000
SEED_F = 3     # visualSLAM::FmatThresholding: ransacSeed + 3


@pytest.fixture(scope="module")
def pair():
    """the default synth.Scene at the first pose of the corridor trajectory (the pair of tests/test_gpu_match.py), 640 x 240"""
    R, t = synth.corridor_trajectory(3, step=0.5)[0]
    left, right, _ = synth.Scene().stereo(R, t, K=K4_SMALL, size=(640, 240))
    assert left.shape == (240, 640, 3)
    return left, right


@pytest.fixture(scope="module")
def chain(pair, ctx):
    feats = ctx.sift_extract(list(pair), dict(n_features=N_FEATURES), cap=40000, descriptors=False)
    xy = [f[0] for f in feats]
    got = ctx.brief_describe(list(pair), xy, 32)
    kxy = [xy[i][got[i][1]] for i in range(2)]
    idx, dist = ctx.knn_match(got[0][0], got[1][0], k=2, norm=capi.MATCH_L2_U8)
    return xy, got, kxy, ctx.ratio_pairs(idx, dist, kxy[0], kxy[1], 0.8)


def test_chain_equals_the_cpu_composition(pair, chain, orc):
    xy, got, kxy, (a, b, mask) = chain
    table = capi.brief_default_pattern(32)
    ref = [bn.describe(im, p, table, 32) for im, p in zip(pair, xy)]
    for k in range(2):
        assert_same(got[k], ref[k], f"image {k}")
    idx, dist = mn.knn_match(ref[0][0], ref[1][0], 2, mn.L2_U8)
    ca, cb, cmask = mn.ratio_pairs(idx, dist, xy[0][ref[0][1]], xy[1][ref[1][1]], 0.8)
    assert np.array_equal(a, ca) and np.array_equal(b, cb) and np.array_equal(mask, cmask)
    # the condition on the input: the CPU composition leaves at least 8 F-inliers
    cnt, fmask, _, _ = orc.fransac(ca, cb, 3.0, 0.99, 1000, seed=SEED_F)
    ai, bi = ca[fmask != 0], cb[fmask != 0]
    xyz, _ = orc.triangulate(*orc.stereo_projections(*K4_SMALL, synth.KITTI_BASELINE), ai, bi)
    print(f"SIFT + BRIEF stereo chain at 640 x 240: {len(xy[0])} / {len(xy[1])} SIFT key points, {len(ref[0][1])} / {len(ref[1][1])} "
          f"described, {len(ca)} pairs after the ratio test, {cnt} F-inliers, {np.mean(np.abs(ai[:, 1] - bi[:, 1]) <= 2):.3f} of them "
          f"within 2 px of their row, {np.mean(xyz[:, 2] > 0):.3f} with positive depth")
    assert cnt >= 8


def test_smoke_program_reproduces_the_chain(tmp_path, pair, chain, ctx):
    from test_brief_abi import build_smoke

    _, _, kxy, (a, b, _) = chain
    cnt, fmask, _, _ = ctx.fransac(a, b, 3.0, 0.99, 1000, seed=SEED_F)
    ai, bi = ctx.compact(fmask, a, b)
    P1, P2 = capi.stereo_projections(*K4_SMALL, synth.KITTI_BASELINE)
    xyz, _ = ctx.triangulate(P1, P2, ai, bi)
    pyr = ctx.pyramid(640, 240, 3, 1).build(pair[0])
    colours = ctx.get_colors(pyr, ai)
    pyr.close()
    exe = tmp_path / "brief_stereo_smoke"
    build_smoke(exe)
    files = [str(tmp_path / "left.ppm"), str(tmp_path / "right.ppm")]
    for f, im in zip(files, pair):
        sequence.write_image(f, im)
    run = subprocess.run([str(exe), *files, *(repr(v) for v in K4_SMALL), repr(synth.KITTI_BASELINE), str(N_FEATURES)],
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    lines = run.stdout.splitlines()
    heads = [i for i, line in enumerate(lines) if line.startswith("#")]
    assert len(heads) == 3
    n_pairs, n_in = int(lines[heads[0]].split()[2]), int(lines[heads[1]].split()[2])
    rows = lambda lo, hi, k: np.array([[float(v) for v in line.split()] for line in lines[lo:hi]], np.float64).reshape(-1, k).astype(np.float32)   # noqa: E731
    p = rows(heads[0] + 1, heads[1], 4)
    q = rows(heads[1] + 1, heads[2], 10)
    assert n_pairs == len(a) == len(p) and np.array_equal(p, np.c_[a, b])
    assert n_in == cnt == len(q) and np.array_equal(q[:, :4], np.c_[ai, bi])
    assert np.array_equal(q[:, 4:7], xyz, equal_nan=True) and np.array_equal(q[:, 7:], colours)
    assert lines[heads[2]].split()[2:] == [str(len(kxy[0])), "of", str(len(chain[0][0]))]
