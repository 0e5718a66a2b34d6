"""svo_gftt_detect_batch and svo_gftt_response (csrc/gftt.hip) against the numpy restatement (tests/gftt_numpy.py), bit for bit: the
measure plane, counts, corners in order and responses on every fixture; the seams of the tiles, of the candidate spans, of the sort
and of the selection workgroup; grey and BGR, masks, host and device memory behind guard bands, a batch of 16; capacity; every
refusal; scratch reuse; determinism; the neighbours on the same context; the adaptor's smoke program and stereoTriangulate's GFTT
branch against the same calls issued through capi.  Every comparison is exact."""
import ctypes as C
import pathlib
import re
import subprocess

import numpy as np
import pytest

import gftt_fixtures as gf
import gftt_numpy as gn
from ros_stereo_slam_amd import capi

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parents[1]
CASES = gf.all_cases()
PLAN = (ROOT / "ros_stereo_slam_amd" / "csrc" / "gftt_plan.hip.h").read_text()


def constant(name):
    m = re.search(rf"constexpr int {name} = (\d+);", PLAN)
    assert m, f"gftt_plan.hip.h no longer defines {name}"
    return int(m.group(1))


TILE_W, TILE_H, SPAN, WAVES, SORT_TILE, SELECT_T = (constant(n) for n in ("TILE_W", "TILE_H", "SPAN", "WAVES", "SORT_TILE", "SELECT_T"))
WAVE = 64


def same(got, exp, what):
    assert len(got[0]) == len(exp[0]), (what, len(got[0]), len(exp[0]))
    assert got[0].dtype == np.float32 and got[1].dtype == np.float32
    assert np.array_equal(got[0], exp[0]), (what, "xy")
    assert np.array_equal(got[1].view(np.uint32), exp[1].view(np.uint32)), (what, "response")


def same_plane(got, exp, what):
    assert got.dtype == np.float32 and got.shape == exp.shape
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32)), (what, int((got.view(np.uint32) != exp.view(np.uint32)).sum()))


def plane_params(p):
    return {k: v for k, v in p.items() if k in ("block_size", "use_harris", "k")}


@pytest.mark.parametrize("name", sorted(CASES))
def test_parity_on_every_fixture(ctx, name):
    k = CASES[name]
    same_plane(ctx.gftt_response(k["img"], **plane_params(k["params"])), gn.response(k["img"], **plane_params(k["params"])), name)
    got = ctx.gftt_detect([k["img"]], None if k["mask"] is None else [k["mask"]], **k["params"])[0]
    same(got, gf.expected(name), name)


@pytest.mark.parametrize("name", ["min_distance_10", "mask_hides_maximum", "harris_block5_bgr", "plateau_min_distance", "three_by_three",
                                  "two_by_five", "selection_chain"])
def test_device_memory_equals_host_memory(ctx, name):
    import torch

    k = CASES[name]
    img = torch.from_numpy(k["img"]).cuda()
    mask = None if k["mask"] is None else [torch.from_numpy(k["mask"]).cuda()]
    same(ctx.gftt_detect([img], mask, **k["params"])[0], gf.expected(name), name)
    same_plane(ctx.gftt_response(img, **plane_params(k["params"])), gn.response(k["img"], **plane_params(k["params"])), name)


def test_tile_seams(ctx):
    """Widths and heights one less than, equal to, one more than and one more than twice the eig launch's tile, grey and BGR,
    block sizes 3 and 7, planes around the 1024 pixels a wavefront of the candidate launches owns"""
    sizes = [(w, h) for w in (TILE_W - 1, TILE_W, TILE_W + 1, 2 * TILE_W + 1) for h in (TILE_H - 1, TILE_H, TILE_H + 1, 2 * TILE_H + 1)]
    sizes += [(31, 33), (32, 32), (41, 25)]
    assert (31 * 33, 32 * 32, 41 * 25) == (SPAN - 1, SPAN, SPAN + 1)
    for j, (w, h) in enumerate(sizes):
        img = gf.noise(w, h, 400 + j, channels=3 if j % 3 == 0 else 1)
        for bs in (3, 7):
            same_plane(ctx.gftt_response(img, block_size=bs), gn.response(img, bs), (w, h, bs))
        exp = gn.detect(img, max_corners=0, min_distance=3.0, block_size=3 + 4 * (j % 2))
        same(ctx.gftt_detect([img], max_corners=0, min_distance=3.0, block_size=3 + 4 * (j % 2))[0], exp, (w, h))
        assert len(exp[0]) > 0, (w, h)


def test_small_images_under_the_largest_block(ctx):
    """Images smaller than the halo of a 31 x 31 window: the mirrored border folds more than once"""
    for j, (w, h) in enumerate([(1, 1), (1, 9), (2, 2), (3, 3), (5, 4), (9, 40), (17, 17)]):
        img = gf.noise(w, h, 450 + j)
        for bs in (3, 15, 31):
            same_plane(ctx.gftt_response(img, block_size=bs), gn.response(img, bs), (w, h, bs))


@pytest.mark.parametrize("n", sorted({WAVE - 1, WAVE, WAVE + 1, 64 * WAVES - 1, 64 * WAVES, 64 * WAVES + 1, SELECT_T - 1, SELECT_T, SELECT_T + 1,
                                      SORT_TILE - 1, SORT_TILE, SORT_TILE + 1}))
def test_candidate_count_seams(ctx, n):
    """Exactly n candidates, 50 distinct values among them: a wavefront, a candidate workgroup, the selection workgroup and a tile of
    the radix sort, one less and one more"""
    img = gf.dot_lattice(n)
    for md in (0.0, 7.0):
        exp = gn.detect(img, max_corners=0, quality_level=0.1, min_distance=md)
        assert exp[2]["n_candidates"] == n and exp[2]["ties"] >= n - 50
        same(ctx.gftt_detect([img], max_corners=0, quality_level=0.1, min_distance=md)[0], exp, (n, md))
        assert md == 0 or 0 < len(exp[0]) < n


def test_more_spans_than_one_chunk_of_the_scan(ctx):
    """520 x 512 = 260 spans of 1024 pixels: the scan of the span counts (256 a chunk) takes a second chunk; two images, so that the
    second image's candidates start behind the first's"""
    w, h = 520, 512
    assert w * h == 260 * SPAN and 260 > 256
    imgs = [gf.noise(w, h, 600), gf.blocks(w, h, 601)]
    got = ctx.gftt_detect(imgs, max_corners=0, min_distance=0.0, quality_level=0.05)
    for j, img in enumerate(imgs):
        exp = gn.detect(img, max_corners=0, min_distance=0.0, quality_level=0.05)
        past = exp[0][:, 1] * w + exp[0][:, 0] >= 256 * SPAN
        assert past.any() and not past.all() and len(exp[0]) > SORT_TILE * (1 - j)
        same(got[j], exp, j)


def test_batch_of_16_equals_16_single_calls(ctx):
    imgs = [gf.noise(75, 41, 100 + k) for k in range(12)] + [gf.blocks(75, 41, 200 + k) for k in range(4)]
    masks = [None if k % 3 else (gf.noise(75, 41, 300 + k) > 60).astype(np.uint8) for k in range(16)]
    for prm in (dict(min_distance=4.0, max_corners=0), dict(min_distance=0.0, max_corners=25), dict(use_harris=1, min_distance=2.0)):
        batch = ctx.gftt_detect(imgs, masks, **prm)
        assert len(batch) == 16
        for k, img in enumerate(imgs):
            same(batch[k], ctx.gftt_detect([img], [masks[k]], **prm)[0], ("single", k))
            q = dict(prm, use_harris=bool(prm.get("use_harris", 0)))
            same(batch[k], gn.detect(img, mask=masks[k], **q), ("restatement", k))
    bgr = [gf.noise(50, 37, 320 + k, channels=3) for k in range(16)]
    for k, got in enumerate(ctx.gftt_detect(bgr, min_distance=5.0)):
        same(got, gn.detect(bgr[k], min_distance=5.0), ("bgr batch", k))


# ------------------------------------------------------------------------------------------------------------- capacity, guard bands
def raw_detect(ctx, imgs, prm, cap, device=False, guard=64):
    """The C call with a guard band behind xy and response -> (rc, n, xy, resp) as host arrays with the bands attached"""
    nimg = len(imgs)
    h, w = imgs[0].shape[:2]
    c = 1 if imgs[0].ndim == 2 else imgs[0].shape[2]
    n = (C.c_int * nimg)(*([-1] * nimg))
    if device:
        import torch

        dev = [torch.from_numpy(np.ascontiguousarray(im)).cuda() for im in imgs]
        out = torch.full((nimg * cap * 3 + 2 * guard,), -77.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ptrs = (C.c_void_p * nimg)(*[d.data_ptr() for d in dev])
        rc = ctx.lib.svo_gftt_detect_batch(ctx._h, ptrs, None, nimg, w, h, c, C.byref(prm), cap, C.c_void_p(out.data_ptr()),
                                           C.c_void_p(out.data_ptr() + 4 * (nimg * cap * 2 + guard)), n, capi.MEM_DEVICE)
        ctx.sync()
        host = out.cpu().numpy()
        return rc, list(n), host[:nimg * cap * 2 + guard], host[nimg * cap * 2 + guard:]
    xy = np.full(nimg * cap * 2 + guard, -77.0, np.float32)
    resp = np.full(nimg * cap + guard, -77.0, np.float32)
    ptrs = (C.c_void_p * nimg)(*[im.ctypes.data for im in imgs])
    rc = ctx.lib.svo_gftt_detect_batch(ctx._h, ptrs, None, nimg, w, h, c, C.byref(prm), cap, xy.ctypes.data_as(C.c_void_p),
                                       resp.ctypes.data_as(C.c_void_p), n, capi.MEM_HOST)
    return rc, list(n), xy, resp


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_capacity_and_guard_bands(ctx, device):
    base = CASES["min_distance_10"]["img"]
    imgs = [np.ascontiguousarray(base), np.ascontiguousarray(base[::-1])]
    prm = capi.gftt_params(min_distance=6.0, max_corners=0)
    exp = [gn.detect(im, min_distance=6.0, max_corners=0) for im in imgs]
    needed = [len(e[0]) for e in exp]
    assert min(needed) > 8
    for cap, want_rc in ((max(needed) - 1, capi.SVO_ERR_CAPACITY), (min(needed) - 3, capi.SVO_ERR_CAPACITY), (max(needed), capi.SVO_OK)):
        rc, n, xy, resp = raw_detect(ctx, imgs, prm, cap, device)
        assert rc == want_rc and n == needed, (cap, rc, n, needed)
        for k, e in enumerate(exp):
            m = min(needed[k], cap)
            assert np.array_equal(xy[2 * k * cap:2 * (k * cap + m)].reshape(-1, 2), e[0][:m])
            assert np.array_equal(resp[k * cap:k * cap + m], e[1][:m])
            assert (xy[2 * (k * cap + m):2 * (k + 1) * cap] == -77).all() and (resp[k * cap + m:(k + 1) * cap] == -77).all()
        assert (xy[2 * 2 * cap:] == -77).all() and (resp[2 * cap:] == -77).all()
    with pytest.raises(capi.SvoError) as err:
        ctx.gftt_detect(imgs, params=prm, cap=max(needed) - 1)
    assert err.value.code == capi.SVO_ERR_CAPACITY and err.value.needed == needed
    # max_corners is the count that is reported, not the number of accepted corners behind it
    rc, n, xy, resp = raw_detect(ctx, imgs, capi.gftt_params(min_distance=6.0, max_corners=5), 5, device)
    assert rc == capi.SVO_OK and n == [5, 5] and np.array_equal(xy[:10].reshape(-1, 2), exp[0][0][:5])


def test_every_refusal_with_a_context(ctx):
    lib = ctx.lib
    img = np.ascontiguousarray(CASES["min_distance_10"]["img"])
    h, w = img.shape
    ptrs = (C.c_void_p * 17)(*([img.ctypes.data] * 17))
    good = capi.gftt_params()
    xy, resp = np.full((8192, 2), -5, np.float32), np.full(8192, -5, np.float32)
    n = (C.c_int * 17)(*([-3] * 17))
    X, R = xy.ctypes.data_as(C.c_void_p), resp.ctypes.data_as(C.c_void_p)

    def detect(images=ptrs, nimg=1, w=w, h=h, c=1, prm=good, cap=4, xy_=X, n_=n, mem=capi.MEM_HOST):
        return lib.svo_gftt_detect_batch(ctx._h, images, None, nimg, w, h, c, C.byref(prm) if prm else None, cap, xy_, R, n_, mem)

    nan = float("nan")
    cases = [dict(images=None), dict(prm=None), dict(xy_=None), dict(n_=None), dict(c=0), dict(c=2), dict(c=4), dict(nimg=0), dict(nimg=17),
             dict(nimg=-1), dict(cap=0), dict(cap=-1), dict(w=0), dict(h=0), dict(w=-4), dict(w=16385), dict(h=16385), dict(w=16384, h=16384),
             dict(mem=2)]
    cases += [dict(prm=capi.gftt_params(block_size=b)) for b in (1, 2, 4, 33, -3)]
    cases += [dict(prm=capi.gftt_params(quality_level=q)) for q in (0.0, -0.5, 1.5, nan)]
    cases += [dict(prm=capi.gftt_params(min_distance=d)) for d in (-1.0, nan)]
    cases += [dict(prm=capi.gftt_params(use_harris=1, k=nan))]
    for kw in cases:
        assert detect(**kw) == capi.SVO_ERR_ARG, kw
        assert b"svo_gftt_detect_batch" in lib.svo_last_error(), kw
    assert detect(images=(C.c_void_p * 2)(img.ctypes.data, None), nimg=2) == capi.SVO_ERR_ARG
    assert (xy == -5).all() and (resp == -5).all() and all(v == -3 for v in n), "a refused call wrote something"
    # the legal neighbours of the refusals
    assert detect(cap=8192) == capi.SVO_OK and n[0] > 0
    assert detect(cap=8192, prm=capi.gftt_params(min_distance=float("inf"))) == capi.SVO_OK and n[0] == 1
    assert detect(cap=8192, prm=capi.gftt_params(quality_level=1.0)) == capi.SVO_OK and n[0] == 0
    assert detect(cap=8192, prm=capi.gftt_params(block_size=31, max_corners=-5, min_distance=0.0)) == capi.SVO_OK and n[0] > 0
    small = np.zeros((5, 2), np.uint8)
    assert detect(images=(C.c_void_p * 1)(small.ctypes.data), w=2, h=5) == capi.SVO_OK and n[0] == 0


def test_scratch_is_reused_from_a_large_image_to_a_small_one(ctx):
    big, small = gf.noise(300, 200, 700), CASES["tie_inside_min_distance"]
    exp_big = gn.detect(big, min_distance=12.0, max_corners=0)
    for _ in range(2):
        same(ctx.gftt_detect([big] * 3, min_distance=12.0, max_corners=0)[2], exp_big, "big")
        same(ctx.gftt_detect([small["img"]], **small["params"])[0], gf.expected("tie_inside_min_distance"), "small after big")
        same(ctx.gftt_detect([CASES["flat"]["img"]])[0], gf.expected("flat"), "flat after big")


def blob(res):
    return b"".join(a.tobytes() for r in res for a in r)


def test_five_runs_and_two_contexts_give_identical_bytes(ctx):
    imgs = [CASES["block7_blocks"]["img"], gf.blocks(160, 96, 77), gf.noise(160, 96, 78)]

    def run(c):
        return (blob(c.gftt_detect(imgs, min_distance=5.0)) + blob(c.gftt_detect(imgs, min_distance=0.0, use_harris=1, max_corners=0))
                + c.gftt_response(imgs[0], block_size=5).tobytes())

    runs = [run(ctx) for _ in range(5)]
    assert all(r == runs[0] for r in runs[1:]) and len(runs[0]) > 160 * 96 * 4
    other = capi.Context(0)
    try:
        assert run(other) == runs[0]
    finally:
        other.close()


def test_fast_and_anms_are_undisturbed(ctx):
    frame = gf.blocks(160, 96, 90)
    rng = np.random.default_rng(3)
    pts, resp = (rng.random((900, 2)) * 600).astype(np.float32), rng.random(900).astype(np.float32)

    def neighbours():
        return blob(ctx.fast_detect([frame, frame[:, ::-1].copy()], 5, True, score=True)) + ctx.anms(pts, resp, 200).tobytes()

    before = neighbours()
    ctx.gftt_detect([frame], min_distance=10.0)
    ctx.gftt_detect([gf.noise(50, 37, 91, channels=3)] * 16, min_distance=0.0, use_harris=1)
    ctx.gftt_response(frame, block_size=31)
    assert neighbours() == before and len(before) > 2 * 160 * 96


# ------------------------------------------------------------------------------------------------------------- the adaptor
def test_gftt_smoke_and_stereo_triangulate_equal_the_python_path(ctx, tmp_path):
    from ros_stereo_slam_amd import sequence, synth
    from test_gftt_abi import build_smoke

    K4 = (360.0, 360.0, 320.0, 120.0)
    sc = synth.Scene()
    R, t = synth.corridor_trajectory(1)[0]
    left, right = sc.stereo(R, t, K=K4, size=(640, 240))[:2]
    left, right = np.ascontiguousarray(left), np.ascontiguousarray(right)
    assert left.ndim == 3 and left.shape[2] == 3
    exe = tmp_path / "gftt_smoke"
    build_smoke(exe)
    files = [str(tmp_path / "left.ppm"), str(tmp_path / "right.ppm")]
    for f, im in zip(files, (left, right)):
        sequence.write_image(f, im)
    mc, q, md = 300, 0.02, 8.0
    run = subprocess.run([str(exe), *files, *(repr(v) for v in K4), repr(synth.KITTI_BASELINE), str(mc), repr(q), repr(md)],
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "gftt smoke ok" in run.stdout, (run.returncode, run.stdout[-2000:], run.stderr)
    sections, name = {}, None
    for line in run.stdout.splitlines():
        if line.startswith("# "):
            name = line.split()[1]
            sections[name] = []
        elif name and line[0] in "-0123456789":
            sections[name].append([float(v) for v in line.split()])
    kps, on = np.array(sections["gftt"], np.float32), np.array(sections["on"], np.float32)
    # the program's key points are the library's through capi, and those are the restatement's
    xy, resp = ctx.gftt_detect([left], max_corners=mc, quality_level=q, min_distance=md)[0]
    assert np.array_equal(kps[:, :2], xy) and np.array_equal(kps[:, 2], resp) and 8 <= len(xy) <= mc
    same((xy, resp), gn.detect(left, max_corners=mc, quality_level=q, min_distance=md), "restatement")
    # stereoTriangulate's GFTT branch = gftt_detect -> LK -> F-RANSAC (3 px, seed ransacSeed + 3) -> svo_triangulate
    pa, pb = capi.Pyramid(ctx, 640, 240, 3).build(left), capi.Pyramid(ctx, 640, 240, 3).build(right)
    trk, status, _, _ = ctx.lk_track(pa, pb, xy)
    ref, trk = xy[status == 1], trk[status == 1]
    _, mask, _, _ = ctx.fransac(ref, trk, 3.0, 0.99, 1000, seed=5 + 3)
    ref, trk = ref[mask == 1], trk[mask == 1]
    P1, P2 = capi.stereo_projections(*K4, synth.KITTI_BASELINE)
    xyz, _ = ctx.triangulate(P1, P2, ref, trk)
    assert len(on) >= 8 and np.array_equal(on[:, :2], ref) and np.array_equal(on[:, 2:], xyz)
    assert (on[:, 4] > 0).all()
