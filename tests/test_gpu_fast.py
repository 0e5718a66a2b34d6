"""svo_fast_detect_batch and svo_fast_anms_batch (csrc/fast.hip) against the numpy restatement (tests/fast_numpy.py), bit for bit:
counts, key points, responses and the score plane on every fixture; the tile seams; capacity; determinism; the chained call against
detect + svo_anms + gather and against the oracle's ANMS; every refusal; the neighbours on the same context; the adaptor's smoke
program.  Every comparison is exact."""
import ctypes as C
import functools
import pathlib
import subprocess

import numpy as np
import pytest

import fast_fixtures as ff
import fast_numpy as fn
from ros_stereo_slam_amd import capi

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parents[1]
FIX = ff.all_fixtures()
# csrc/fast_plan.hip.h: the score launch's tile, and the pixels one wavefront of the compaction owns
TILE_W, TILE_H, SPAN = 64, 16, 1024
THRESHOLDS = (0, 1, 10, 255)


def test_constants_are_the_kernels():
    text = (ROOT / "ros_stereo_slam_amd" / "csrc" / "fast_plan.hip.h").read_text()
    assert f"TILE_W = {TILE_W}, TILE_H = {TILE_H};" in text and f"SPAN = {SPAN}," in text


@functools.lru_cache(maxsize=None)
def want(name, t, nonmax, budget):
    return fn.fast_detect(FIX[name], t, nonmax, budget)


def tie_budget(name, t):
    """A budget whose cut lands on a tie (the k-th and (k + 1)-th largest responses are equal); 2 where the image has no tie."""
    s = np.sort(want(name, t, True, 0)[1])[::-1]
    ks = [k for k in range(1, len(s)) if s[k - 1] == s[k]]
    return ks[len(ks) // 2] if ks else 2


def same(got, exp, what):
    assert len(got[0]) == len(exp[0]), (what, len(got[0]), len(exp[0]))
    assert got[0].dtype == np.float32 and got[1].dtype == np.float32
    assert np.array_equal(got[0], exp[0]), (what, "xy")
    assert np.array_equal(got[1], exp[1]), (what, "response")
    if len(got) > 2:
        assert np.array_equal(got[2], exp[2]), (what, "score plane")


@pytest.mark.parametrize("name", sorted(FIX))
def test_parity_on_every_fixture(ctx, name):
    img = FIX[name]
    for t in THRESHOLDS:
        for nonmax in (True, False):
            for budget in (0, 1, tie_budget(name, t)):
                got = ctx.fast_detect([img], t, nonmax, budget, score=True)[0]
                same(got, want(name, t, nonmax, budget), (name, t, nonmax, budget))
    assert name in ("flat_40x30", "no_interior_20x6", "no_interior_6x20") or len(want(name, 1, False, 0)[0]) > 0


def test_retain_best_cut_on_a_tie_returns_more_than_the_budget(ctx):
    name = "blocks_160x120"
    k = tie_budget(name, 10)
    got = ctx.fast_detect([FIX[name]], 10, True, k)[0]
    assert len(got[0]) > k
    same(got, want(name, 10, True, k), "tie")


@pytest.mark.parametrize("name", ["noise_64x48", "bgr_50x37", "odd_67x35", "blocks_160x120", "one_corner_7x7", "no_interior_6x20"])
def test_device_memory_equals_host_memory(ctx, name):
    import torch

    img = FIX[name]
    dev = torch.from_numpy(img).cuda()
    for t, nonmax, budget in ((1, True, 0), (10, False, 0), (1, True, tie_budget(name, 1)), (0, True, 1)):
        got = ctx.fast_detect([dev], t, nonmax, budget, score=True)[0]
        same(got, want(name, t, nonmax, budget), (name, t, nonmax, budget))


def test_unaligned_grey_device_image_is_read_through_the_grey_plane(ctx):
    """A single-channel device image at an odd address with rows of whole dwords: the in-place path must not be taken."""
    import torch

    img = ff.noise(64, 40, 31)
    buf = torch.zeros(img.size + 8, dtype=torch.uint8, device="cuda")
    for shift in (0, 1, 2, 3):
        view = buf[shift:shift + img.size].view(40, 64)
        view.copy_(torch.from_numpy(img))
        assert view.data_ptr() % 4 == shift
        got = ctx.fast_detect([view], 1, True, score=True)[0]
        same(got, fn.fast_detect(img, 1, True), shift)


def test_batch_of_16_equals_16_single_calls(ctx):
    imgs = [ff.noise(75, 41, 100 + k) for k in range(12)] + [ff.blocks(75, 41, 200 + k) for k in range(4)]
    for t, nonmax, budget in ((1, True, 0), (10, False, 0), (1, True, 7)):
        batch = ctx.fast_detect(imgs, t, nonmax, budget, score=True)
        assert len(batch) == 16
        for k, img in enumerate(imgs):
            single = ctx.fast_detect([img], t, nonmax, budget, score=True)[0]
            same(batch[k], single, ("batch", k))
            same(batch[k], fn.fast_detect(img, t, nonmax, budget), ("restatement", k))
    bgr = [ff.noise(50, 37, 300 + k, channels=3) for k in range(16)]
    for k, got in enumerate(ctx.fast_detect(bgr, 1, True, score=True)):
        same(got, fn.fast_detect(bgr[k], 1, True), ("bgr batch", k))


def test_tile_seams(ctx):
    """Widths and heights one less than, equal to and one more than the score launch's tile (64 x 16), twice the tile on both axes,
    and planes of one pixel less than, exactly, and one more than the 1024 pixels a wavefront of the compaction owns."""
    sizes = [(w, h) for w in (TILE_W - 1, TILE_W, TILE_W + 1) for h in (TILE_H - 1, TILE_H, TILE_H + 1)]
    sizes += [(2 * TILE_W - 1, 2 * TILE_H + 1), (2 * TILE_W, 2 * TILE_H), (2 * TILE_W + 7, 2 * TILE_H + 7)]
    sizes += [(SPAN // 8 - 1, 8), (SPAN // 8, 8), (SPAN // 8 + 1, 8), (31, 33), (32, 32), (41, 25)]
    assert (31 * 33, 32 * 32, 41 * 25) == (SPAN - 1, SPAN, SPAN + 1)
    for k, (w, h) in enumerate(sizes):
        for img in (ff.noise(w, h, 400 + k), ff.noise(w, h, 500 + k, channels=3)):
            for t, nonmax in ((1, True), (0, False)):
                exp = fn.fast_detect(img, t, nonmax)
                same(ctx.fast_detect([img], t, nonmax, score=True)[0], exp, (w, h, img.ndim, t, nonmax))
            assert len(exp[0]) > 0, (w, h)


def test_more_spans_than_one_chunk_of_the_scan(ctx):
    """520 x 512 = 260 spans of 1024 pixels: the scan of the span counts (256 a chunk) takes a second chunk, whose offsets start from
    the first one's carry; with a budget the count / scan pair runs twice.  Key points lie on both sides of the seam."""
    w, h = 520, 512
    assert w * h == 260 * SPAN and 260 > 256
    img = ff.noise(w, h, 600)
    for t, nonmax, budget in ((1, True, 0), (10, True, 500)):
        exp = fn.fast_detect(img, t, nonmax, budget)
        past = exp[0][:, 1] * w + exp[0][:, 0] >= 256 * SPAN
        assert past.any() and not past.all()
        same(ctx.fast_detect([img], t, nonmax, budget)[0], exp, (t, nonmax, budget))


# ------------------------------------------------------------------------------------------------------------- capacity
def raw_detect(ctx, imgs, prm, cap, guard=64):
    """The C call on host arrays with a guard band behind xy and response -> (rc, n, xy, resp) with the bands attached."""
    nimg = len(imgs)
    h, w = imgs[0].shape[:2]
    c = 1 if imgs[0].ndim == 2 else imgs[0].shape[2]
    xy = np.full(nimg * cap * 2 + guard, -77.0, np.float32)
    resp = np.full(nimg * cap + guard, -77.0, np.float32)
    n = (C.c_int * nimg)(*([-1] * nimg))
    ptrs = (C.c_void_p * nimg)(*[im.ctypes.data for im in imgs])
    rc = ctx.lib.svo_fast_detect_batch(ctx._h, ptrs, nimg, w, h, c, C.byref(prm), cap, xy.ctypes.data_as(C.c_void_p),
                                       resp.ctypes.data_as(C.c_void_p), None, n, capi.MEM_HOST)
    return rc, list(n), xy, resp


def test_capacity(ctx):
    imgs = [np.ascontiguousarray(FIX["noise_64x48"]), np.ascontiguousarray(FIX["noise_64x48"][::-1])]
    exp = [fn.fast_detect(im, 1, True) for im in imgs]
    needed = [len(e[0]) for e in exp]
    cap = max(needed) - 1
    assert min(needed) > 8 and cap >= 1
    prm = capi.fast_params(threshold=1)
    rc, n, xy, resp = raw_detect(ctx, imgs, prm, cap)
    assert rc == capi.SVO_ERR_CAPACITY and n == needed
    for k, e in enumerate(exp):
        m = min(needed[k], cap)
        assert np.array_equal(xy[2 * k * cap:2 * (k * cap + m)].reshape(-1, 2), e[0][:m])
        assert np.array_equal(resp[k * cap:k * cap + m], e[1][:m])
        # the slots between an image's count and cap are untouched too
        assert (xy[2 * (k * cap + m):2 * (k + 1) * cap] == -77).all() and (resp[k * cap + m:(k + 1) * cap] == -77).all()
    assert (xy[2 * 2 * cap:] == -77).all() and (resp[2 * cap:] == -77).all()
    with pytest.raises(capi.SvoError) as err:
        ctx.fast_detect(imgs, 1, True, cap=cap)
    assert err.value.code == capi.SVO_ERR_CAPACITY and err.value.needed == needed
    # device memory: nothing past cap either
    import torch

    dev = [torch.from_numpy(im).cuda() for im in imgs]
    out = torch.full((2 * cap * 3 + 64,), -77.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    nd = (C.c_int * 2)(-1, -1)
    ptrs = (C.c_void_p * 2)(*[d.data_ptr() for d in dev])
    rc = ctx.lib.svo_fast_detect_batch(ctx._h, ptrs, 2, 64, 48, 1, C.byref(prm), cap, C.c_void_p(out.data_ptr()),
                                       C.c_void_p(out.data_ptr() + 8 * 2 * cap), None, nd, capi.MEM_DEVICE)
    ctx.sync()
    host = out.cpu().numpy()
    assert rc == capi.SVO_ERR_CAPACITY and list(nd) == needed and (host[2 * cap * 3:] == -77).all()
    for k, e in enumerate(exp):
        m = min(needed[k], cap)
        assert np.array_equal(host[2 * k * cap:2 * (k * cap + m)].reshape(-1, 2), e[0][:m])
        assert np.array_equal(host[4 * cap + k * cap:4 * cap + k * cap + m], e[1][:m])
    # a later call with enough room is correct
    rc, n, xy, resp = raw_detect(ctx, imgs, prm, max(needed))
    assert rc == capi.SVO_OK and n == needed
    for k, got in enumerate(ctx.fast_detect(imgs, 1, True, cap=max(needed), score=True)):
        same(got, exp[k], ("after overflow", k))


# ------------------------------------------------------------------------------------------------------------- determinism
def blob(res):
    return b"".join(a.tobytes() for r in res for a in r)


def test_five_runs_and_two_contexts_give_identical_bytes(ctx):
    imgs = [FIX["blocks_160x120"], ff.blocks(160, 120, 77), ff.noise(160, 120, 78)]
    runs = [blob(ctx.fast_detect(imgs, 1, True, 40, score=True)) + blob(ctx.fast_anms(imgs, 50, 1)) for _ in range(5)]
    assert all(r == runs[0] for r in runs[1:]) and len(runs[0]) > 3 * 160 * 120
    other = capi.Context(0)
    try:
        assert blob(other.fast_detect(imgs, 1, True, 40, score=True)) + blob(other.fast_anms(imgs, 50, 1)) == runs[0]
    finally:
        other.close()


# ------------------------------------------------------------------------------------------------------------- the chained call
def test_fast_anms_equals_detect_anms_gather_and_the_oracle(ctx, orc):
    imgs = [FIX["blocks_160x120"], ff.noise(160, 120, 78), np.full((120, 160), 9, np.uint8)]
    det = ctx.fast_detect(imgs, 10, True)
    counts = [len(d[0]) for d in det]
    assert counts[0] > 100 and counts[1] > 100 and counts[2] == 0
    for keep in (1, 37, counts[0] - 1, counts[0], counts[0] + 1, counts[1], 100000):
        got = ctx.fast_anms(imgs, keep, 10)
        for k, (xy, resp) in enumerate(det):
            exp_xy, exp_r, _ = fn.fast_detect(imgs[k], 10, True)
            assert np.array_equal(xy, exp_xy) and np.array_equal(resp, exp_r)
            idx = ctx.anms(xy, resp, keep)
            assert np.array_equal(got[k][0], xy[idx]) and np.array_equal(got[k][1], resp[idx]), (keep, k)
            oidx, _ = orc.anms(exp_xy, exp_r, keep)
            assert np.array_equal(got[k][0], exp_xy[oidx]) and np.array_equal(got[k][1], exp_r[oidx]), (keep, k)
            assert len(oidx) == (len(exp_xy) if len(exp_xy) <= keep else len(oidx)) and (len(exp_xy) <= keep or len(oidx) >= keep)
    # device memory, a BGR image, no suppression (every response 0: ANMS keeps input order among ties)
    import torch

    bgr = FIX["bgr_blocks_64x40"]
    for nonmax in (True, False):
        xy, resp = ctx.fast_detect([bgr], 1, nonmax)[0]
        idx = ctx.anms(xy, resp, 20)
        got = ctx.fast_anms([torch.from_numpy(bgr).cuda()], 20, 1, nonmax)[0]
        assert len(xy) > 20 and np.array_equal(got[0], xy[idx]) and np.array_equal(got[1], resp[idx])


def test_fast_anms_overflow_runs_no_anms(ctx):
    img = FIX["noise_64x48"]
    needed = len(fn.fast_detect(img, 1, True)[0])
    with pytest.raises(capi.SvoError) as err:
        ctx.fast_anms([img], 5, 1, cap=needed - 1)
    assert err.value.code == capi.SVO_ERR_CAPACITY and err.value.needed == [needed]
    got = ctx.fast_anms([img], 5, 1, cap=needed)[0]
    xy, resp = ctx.fast_detect([img], 1)[0]
    idx = ctx.anms(xy, resp, 5)
    assert np.array_equal(got[0], xy[idx]) and np.array_equal(got[1], resp[idx])


# ------------------------------------------------------------------------------------------------------------- refusals
def test_every_refusal(ctx):
    lib = ctx.lib
    img = np.ascontiguousarray(FIX["noise_64x48"])
    ptrs = (C.c_void_p * 17)(*([img.ctypes.data] * 17))
    good = capi.fast_params()
    xy, resp = np.full((4096, 2), -5, np.float32), np.full(4096, -5, np.float32)         # room for the legal calls at the end
    n = (C.c_int * 17)(*([-3] * 17))
    X, R = xy.ctypes.data_as(C.c_void_p), resp.ctypes.data_as(C.c_void_p)

    def detect(images=ptrs, nimg=1, w=64, h=48, c=1, prm=good, cap=4, xy_=X, n_=n, mem=capi.MEM_HOST, ctx_h=None):
        return lib.svo_fast_detect_batch(ctx._h if ctx_h is None else ctx_h, images, nimg, w, h, c, C.byref(prm) if prm else None, cap,
                                         xy_, R, None, n_, mem)

    def chain(images=ptrs, nimg=1, w=64, h=48, c=1, prm=good, keep=5, cap=4, xy_=X, n_=n, mem=capi.MEM_HOST):
        return lib.svo_fast_anms_batch(ctx._h, images, nimg, w, h, c, C.byref(prm) if prm else None, keep, cap, xy_, R, n_, mem)

    for call in (detect, chain):
        cases = [dict(images=None), dict(prm=None), dict(xy_=None), dict(n_=None), dict(c=0), dict(c=2), dict(c=4), dict(nimg=0),
                 dict(nimg=17), dict(nimg=-1), dict(cap=0), dict(cap=-1), dict(w=0), dict(h=0), dict(w=-4), dict(w=16385), dict(h=16385),
                 dict(prm=capi.fast_params(threshold=-1)), dict(prm=capi.fast_params(threshold=256)),
                 dict(prm=capi.fast_params(max_keypoints=-1)), dict(mem=2)]
        for kw in cases:
            assert call(**kw) == capi.SVO_ERR_ARG, (call.__name__, kw)
            name = b"svo_fast_detect_batch" if call is detect else b"svo_fast_anms_batch"
            assert name in lib.svo_last_error(), (call.__name__, kw, lib.svo_last_error())
    for keep in (0, -1):
        assert chain(keep=keep) == capi.SVO_ERR_ARG
    null_img = (C.c_void_p * 2)(img.ctypes.data, None)
    assert detect(images=null_img, nimg=2) == capi.SVO_ERR_ARG
    assert (xy == -5).all() and (resp == -5).all() and all(v == -3 for v in n), "a refused call wrote something"
    # the legal neighbours of the refusals
    assert detect(cap=64) in (capi.SVO_OK, capi.SVO_ERR_CAPACITY)
    small = np.zeros((6, 6), np.uint8)
    sp = (C.c_void_p * 1)(small.ctypes.data)
    assert detect(images=sp, w=6, h=6) == capi.SVO_OK and n[0] == 0        # legal, no key points
    assert detect(images=sp, w=1, h=1) == capi.SVO_OK and n[0] == 0
    assert chain(images=sp, w=6, h=6) == capi.SVO_OK and n[0] == 0
    assert detect(prm=capi.fast_params(threshold=255), cap=64) == capi.SVO_OK and n[0] == 0
    assert detect(prm=capi.fast_params(threshold=0), cap=4096) == capi.SVO_OK and n[0] > 0


# ------------------------------------------------------------------------------------------------------------- neighbours
def test_orb_and_anms_are_undisturbed(ctx):
    from ros_stereo_slam_amd import synth

    sc = synth.Scene()
    R, t = synth.corridor_trajectory(1)[0]
    frame = sc.stereo(R, t, K=(360.0, 360.0, 320.0, 120.0), size=(640, 240))[0]
    rng = np.random.default_rng(3)
    pts, resp = (rng.random((900, 2)) * 600).astype(np.float32), rng.random(900).astype(np.float32)

    def neighbours():
        orb = ctx.orb_extract_batch([frame, frame[:, ::-1].copy()], n_features=300)
        return blob(orb) + ctx.anms(pts, resp, 200).tobytes()

    before = neighbours()
    ctx.fast_detect([frame], 1, True, 50, score=True)
    ctx.fast_anms([frame, frame], 300, 5)
    ctx.fast_detect([FIX["bgr_50x37"]] * 16, 0, False)
    assert neighbours() == before and len(before) > 10000


# ------------------------------------------------------------------------------------------------------------- the adaptor
def test_fast_anms_smoke_runs_on_gpu(ctx, tmp_path):
    from ros_stereo_slam_amd import sequence, synth
    from test_fast_abi import build_smoke

    # a fronto-parallel texture at a disparity of 12 pixels (depth fx b / 12): every point has a depth whose sign means something
    K4 = (360.0, 360.0, 320.0, 120.0)
    left, right = synth.textured_pair(640, 240, 3, shift=(-12.0, 0.0), seed=4)
    exe = tmp_path / "fast_anms_smoke"
    build_smoke(exe)
    files = [str(tmp_path / "left.ppm"), str(tmp_path / "right.ppm")]
    for f, im in zip(files, (left, right)):
        sequence.write_image(f, im)
    thr, keep = 3, 200
    run = subprocess.run([str(exe), *files, *(repr(v) for v in K4), repr(synth.KITTI_BASELINE), str(thr), str(keep)],
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "fast anms smoke ok" in run.stdout, (run.returncode, run.stdout[-2000:], run.stderr)
    sections, name = {}, None
    for line in run.stdout.splitlines():
        if line.startswith("# "):
            name = line.split()[1]
            sections[name] = []
        elif name and line[0] in "-0123456789":
            sections[name].append([float(v) for v in line.split()])
    fast, anms = np.array(sections["fast"], np.float32), np.array(sections["anms"], np.float32)
    # the program's key points are the library's, and the library's are the restatement's
    exp_xy, exp_r, _ = fn.fast_detect(left, thr, True)
    assert np.array_equal(fast[:, :2], exp_xy) and np.array_equal(fast[:, 2], exp_r)
    got = ctx.fast_anms([left], keep, thr)[0]
    assert np.array_equal(anms[:, :2], got[0]) and np.array_equal(anms[:, 2], got[1]) and 0 < len(anms) < len(fast)
    corners = set(map(tuple, exp_xy.tolist()))
    for key, source in (("on0", corners), ("on1", set(map(tuple, got[0].tolist())))):
        pairs = np.array(sections[key], np.float32)
        assert len(pairs) >= 8 and all(tuple(p) in source for p in pairs[:, :2].tolist()), key
        assert (pairs[:, 4] > 0).all(), key
