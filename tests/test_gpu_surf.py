"""svo_surf_* against the numpy restatement (tests/surf_numpy.py), bit for bit: both sides are specified operation by operation,
so the bar is np.array_equal on every det and trace plane (read through the diagnostics entry svo_surf_layers), the key point
count, the bits of xy / size / angle / response, octave and laplacian, and the descriptors.

End to end: on the rendered stereo pair of tests/test_gpu_brief.py the pairs of SURF -> knn_match -> ratio_pairs equal the CPU
composition (surf_numpy -> match_numpy) pair for pair, and the C++ adaptors (visualOdometry::stereoTriangulate / relocalizeFrames,
the SURF branch of visualSLAM::stereoTriangulate) reproduce the Python path."""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest

import match_numpy as mn
import surf_numpy as sn
from ros_stereo_slam_amd import capi, sequence, synth

pytestmark = pytest.mark.gpu

K4_SMALL = (360.0, 360.0, 320.0, 120.0)
SIZES = {"640x240": ((640, 240), K4_SMALL), "1241x376": ((1241, 376), (718.856, 718.856, 607.1928, 185.2157))}
FIELDS = ("xy", "size", "angle", "response")


@functools.lru_cache(maxsize=None)
def frame(size_key, channels=3, k=0):
    if size_key == "40x40":
        return np.ascontiguousarray(frame("640x240", 1)[100:140, 300:340])
    size, K4 = SIZES[size_key]
    R, t = synth.corridor_trajectory(k + 1, step=0.5)[k]
    img, _ = synth.Scene().render(R, t, K=K4, size=size, channels=channels)
    return np.ascontiguousarray(img if channels == 3 else img.reshape(size[1], size[0]))


@functools.lru_cache(maxsize=None)
def planes(size_key, channels, no, nl):
    return sn.layers(frame(size_key, channels), no, nl)


_described = {}


def restate(img, key, threshold, upright=0, planes_=None):
    """sn.extract with the per-key-point work (angle, descriptor) shared between the thresholds of one image: a threshold only
    selects key points (U6), everything after the detector depends on (x, y, size) alone"""
    kp = sn.detect(img, hessian_threshold=threshold, upright=upright, planes=planes_)
    n = len(kp["size"])
    angle, desc = np.zeros(n, np.float32), np.zeros((n, 64), np.float32)
    ids = [(key, upright, kp["xy"][i].tobytes(), kp["size"][i].tobytes()) for i in range(n)]
    todo = [i for i in range(n) if ids[i] not in _described]
    if todo:
        a, d, kept = sn.compute(img, kp["xy"][todo], kp["size"][todo], upright)
        assert kept.all()
        for j, i in enumerate(todo):
            _described[ids[i]] = (a[j], d[j])
    for i in range(n):
        angle[i], desc[i] = _described[ids[i]]
    kp["angle"], kp["desc"] = angle, desc
    return kp


@functools.lru_cache(maxsize=None)
def restated(size_key, channels, threshold, upright=0):
    return restate(frame(size_key, channels), (size_key, channels), threshold, upright, planes(size_key, channels, 4, 3))


def assert_same(got, ref, what):
    xy, size, angle, resp, octv, lap, desc = got
    assert len(xy) == len(ref["xy"]), f"{what}: {len(xy)} key points, the restatement has {len(ref['xy'])}"
    for name, a in zip(FIELDS, (xy, size, angle, resp)):
        b = ref[name]
        diff = (a.view(np.uint32) != b.view(np.uint32)).reshape(len(a), -1).any(1)
        assert not diff.any(), f"{what}: {name} differs at {int(diff.sum())} key points, first {int(np.flatnonzero(diff)[0])}"
    assert np.array_equal(octv, ref["octave"]), f"{what}: octave differs"
    assert np.array_equal(lap, ref["laplacian"]), f"{what}: laplacian differs"
    if desc is not None:
        bad = np.flatnonzero((desc.view(np.uint32) != ref["desc"].view(np.uint32)).any(1))
        assert len(bad) == 0, (f"{what}: {len(bad)} descriptors differ, first {bad[0]} (size {size[bad[0]]}): entries "
                               f"{np.flatnonzero(desc[bad[0]] != ref['desc'][bad[0]])}")


def same_bits(a, b):
    return all((x is None and y is None) or (x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32)))
               for x, y in zip(a, b))


# ---- planes ----
@pytest.mark.parametrize("size_key,channels,no,nl", [("640x240", 3, 4, 3), ("1241x376", 1, 4, 4), ("40x40", 1, 4, 3)])
def test_every_plane_equals_the_restatement(ctx, size_key, channels, no, nl):
    ref_det, ref_trace = planes(size_key, channels, no, nl)
    det, trace = ctx.surf_layers(frame(size_key, channels), dict(n_octaves=no, n_octave_layers=nl))
    assert len(det) == len(ref_det) == no * (nl + 2)
    sizes, _, lw, lh = sn.layers_layout(*frame(size_key, channels).shape[1::-1], no, nl)
    empty = 0
    for k in range(len(det)):
        assert det[k].shape == ref_det[k].shape == (lh[k], lw[k])
        assert np.array_equal(det[k].view(np.uint32), ref_det[k].view(np.uint32)), f"det of layer {k} (size {sizes[k]}) differs"
        assert np.array_equal(trace[k].view(np.uint32), ref_trace[k].view(np.uint32)), f"trace of layer {k} (size {sizes[k]}) differs"
        fits = sizes[k] <= min(frame(size_key, channels).shape[:2])
        assert fits == bool(ref_det[k].any()), f"layer {k} (size {sizes[k]})"
        empty += not fits
    # 640x240: size 264, the top layer of octave 3, exceeds 240 rows; 40x40: octave 0, 18 and 30 of octave 1 and 36 of octave 2 fit
    assert empty == {"640x240": 1, "1241x376": 0, "40x40": 12}[size_key]


# ---- key points and descriptors ----
@pytest.mark.parametrize("size_key,channels,threshold,upright",
                         [("640x240", 1, 100, 0), ("640x240", 1, 500, 0), ("640x240", 3, 100, 0), ("640x240", 3, 500, 0),
                          ("1241x376", 1, 500, 0), ("640x240", 1, 500, 1)])
def test_key_points_and_descriptors_equal_the_restatement(ctx, size_key, channels, threshold, upright):
    """1241x376: the threshold 500 was chosen on the CPU -- the restatement finds 3864 key points at 100, 2849 at 500"""
    ref = restated(size_key, channels, threshold, upright)
    assert len(ref["xy"]) >= 200
    if size_key == "1241x376":
        assert len(ref["xy"]) <= 3200 and ref["size"].max() >= 200   # windows of several hundred pixels a side are among them
    got = ctx.surf_extract([frame(size_key, channels)], dict(hessian_threshold=threshold, upright=upright), cap=8192)[0]
    assert_same(got, ref, f"{size_key} x {channels}, threshold {threshold}, upright {upright}")
    if upright:
        assert np.all(got[2] == 270)
    detect_only = ctx.surf_extract([frame(size_key, channels)], dict(hessian_threshold=threshold, upright=upright), cap=8192,
                                   descriptors=False)[0]
    assert detect_only[6] is None and same_bits(detect_only[:6], got[:6])


# ---- svo_surf_describe ----
def test_describe_equals_the_extractor_and_the_restatement(ctx):
    img = frame("640x240", 1)
    xy, size, angle, _, _, _, desc = ctx.surf_extract([img], dict(hessian_threshold=500), cap=8192)[0]
    a, d, kept = ctx.surf_describe(img, xy, size)
    assert kept.all() and same_bits((a, d), (angle, desc))
    # moved key points, and some that do not fit: too large, no sample inside, a window below 21 pixels, not finite
    moved = (xy[:300] + np.array([0.37, -1.62], np.float32)).astype(np.float32)
    msize = size[:300].copy()
    extra_xy = np.array([[320, 120], [2, 2], [320, 120], [np.nan, 5], [5, np.inf], [-3, 250], [639.5, 239.5]], np.float32)
    extra_size = np.array([2000, 700, 5, 20, 20, 30, 15], np.float32)
    pxy, psize = np.concatenate([moved, extra_xy]), np.concatenate([msize, extra_size])
    ref_a, ref_d, ref_k = sn.compute(img, pxy, psize)
    a, d, kept = ctx.surf_describe(img, pxy, psize)
    assert np.array_equal(kept, ref_k) and not kept[300:305].any() and kept[:300].sum() >= 250
    assert same_bits((a, d), (ref_a, ref_d))
    assert np.all(a[kept == 0] == -1) and not d[kept == 0].any()
    assert ctx.surf_describe(img, np.zeros((0, 2), np.float32), np.zeros(0, np.float32))[1].shape == (0, 64)


# ---- batches and memory modes ----
def variants(n):
    a, b = frame("640x240", 3), frame("640x240", 3, 1)
    out = [a, b]
    for k in range(2, n):
        base = out[k % 2]
        out.append(np.ascontiguousarray(np.roll(base[::-1] if k % 4 < 2 else base, 17 * k, axis=1)))
    return out[:n]


@pytest.mark.parametrize("n", [2, 16])
def test_batch_equals_single_calls(ctx, n):
    imgs = variants(n)
    prm = dict(hessian_threshold=500)
    batch = ctx.surf_extract(imgs, prm, cap=4096)
    for i, im in enumerate(imgs):
        single = ctx.surf_extract([im], prm, cap=4096)[0]
        assert len(single[0]) >= 200 and same_bits(batch[i], single), f"image {i} of {n}"
    assert_same(batch[0], restated("640x240", 3, 500), "image 0 of the batch")


@pytest.mark.parametrize("channels", [1, 3])
def test_device_memory_equals_host_memory(ctx, channels):
    import torch

    imgs = [frame("640x240", channels), frame("640x240", channels, 1)]
    host = ctx.surf_extract(imgs, dict(hessian_threshold=500), cap=4096)
    dev = ctx.surf_extract([torch.from_numpy(im).cuda() for im in imgs], dict(hessian_threshold=500), cap=4096)
    for i in range(2):
        assert len(host[i][0]) >= 200 and same_bits(host[i], dev[i])


# ---- degenerate images, capacity, refusals ----
def test_degenerate_images_give_no_key_points(ctx):
    rng = np.random.default_rng(4)
    for im in (rng.integers(0, 256, (8, 8), dtype=np.uint8), np.full((240, 640), 200, np.uint8), np.zeros((64, 64, 3), np.uint8),
               rng.integers(0, 256, (1, 1), dtype=np.uint8)):
        got = ctx.surf_extract([im], cap=16)[0]
        assert len(got[0]) == 0 and got[6].shape == (0, 64)


def test_capacity_returns_the_needed_count_and_the_prefix(ctx):
    ref = restated("640x240", 1, 500)
    n = len(ref["xy"])
    with pytest.raises(capi.SvoError) as e:
        ctx.surf_extract([frame("640x240", 1)], dict(hessian_threshold=500), cap=n - 1)
    assert e.value.code == capi.SVO_ERR_CAPACITY and e.value.needed == [n]
    assert_same(e.value.prefix[0], {k: v[:n - 1] for k, v in ref.items()}, "the prefix")
    assert_same(ctx.surf_extract([frame("640x240", 1)], dict(hessian_threshold=500), cap=n)[0], ref, "cap == count")


def raw_extract(ctx, img, w, h, c, prm, cap, out, nimg=1, mem=capi.MEM_HOST, images=True):
    p = lambda a: None if a is None else C.c_void_p(a if isinstance(a, int) else a.ctypes.data)   # noqa: E731
    ptrs = (C.c_void_p * 16)(*([img.ctypes.data] * 16)) if images else None
    return ctx.lib.svo_surf_extract_batch(ctx._h, ptrs, nimg, w, h, c, None if prm is None else C.byref(prm), cap, p(out["xy"]),
                                          p(out["size"]), p(out["angle"]), p(out["response"]), p(out["octave"]), p(out["laplacian"]),
                                          p(out["desc"]), p(out["n"]), mem)


def test_refusals_leave_the_outputs_untouched(ctx):
    img = frame("640x240", 1)
    cap = 2048
    mk = lambda: dict(xy=np.full(2 * cap, -7, np.float32), size=np.full(cap, -7, np.float32), angle=np.full(cap, -7, np.float32),   # noqa: E731
                      response=np.full(cap, -7, np.float32), octave=np.full(cap, -7, np.int32), laplacian=np.full(cap, -7, np.int32),
                      desc=np.full(64 * cap, -7, np.float32), n=np.full(2, -9, np.int32))

    def refused(code=capi.SVO_ERR_ARG, w=640, h=240, c=1, cap_=cap, nimg=1, mem=capi.MEM_HOST, images=True, null=None, odd=None, **prm):
        out = mk()
        keep = {k: v.copy() for k, v in out.items()}
        args = dict(out)
        if null:
            args[null] = None
        if odd:
            args[odd] = out[odd].ctypes.data + 2
        assert raw_extract(ctx, img, w, h, c, capi.surf_params(**prm), cap_, args, nimg, mem, images) == code, (null, odd, prm)
        assert all(np.array_equal(out[k].view(np.uint32), keep[k].view(np.uint32)) for k in out)

    for name in ("xy", "size", "angle", "response", "octave", "laplacian", "n"):
        refused(null=name)
    for name in ("xy", "size", "angle", "response", "octave", "laplacian", "desc", "n"):
        refused(odd=name)
    refused(images=False)
    for c in (0, 2, 4):
        refused(c=c)
    for v in (0, 9, -1):
        refused(n_octaves=v)
        refused(n_octave_layers=v)
    for v in (-1.0, float("nan"), float("inf")):
        refused(hessian_threshold=v)
    refused(extended=1)
    refused(nimg=0)
    refused(nimg=17)
    refused(cap_=0)
    refused(w=0)
    refused(h=0)
    refused(w=16385)
    refused(mem=2)
    refused(w=16384, h=16384)        # 255 w h > 2^31 - 1: decided before the image is looked at
    refused(w=2901, h=2903)          # 255 * 8421603 = 2^31 + 25117
    big = np.full(4, -7, np.float32)
    p = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
    ext = capi.surf_params(extended=1)
    assert ctx.lib.svo_surf_layers(ctx._h, p(img), 640, 240, 1, C.byref(ext), p(big), p(big), capi.MEM_HOST) == capi.SVO_ERR_ARG
    assert ctx.lib.svo_surf_layers(ctx._h, p(img), 16384, 16384, 1, None, p(big), p(big), capi.MEM_HOST) == capi.SVO_ERR_ARG
    kept = np.full(4, 9, np.uint8)
    assert ctx.lib.svo_surf_describe(ctx._h, p(img), 640, 240, 1, C.byref(ext), p(big), p(big), 1, p(big), p(big), p(kept),
                                     capi.MEM_HOST) == capi.SVO_ERR_ARG
    assert ctx.lib.svo_surf_describe(ctx._h, p(img), 640, 240, 2, None, p(big), p(big), 1, p(big), p(big), p(kept),
                                     capi.MEM_HOST) == capi.SVO_ERR_ARG
    assert np.all(big == -7) and np.all(kept == 9)
    # the same arguments, accepted; a null params pointer means the defaults
    out = mk()
    assert raw_extract(ctx, img, 640, 240, 1, None, cap, out) == capi.SVO_OK
    ref = restated("640x240", 1, 100)
    n = len(ref["xy"])
    assert out["n"][0] == n and out["n"][1] == -9 and np.all(out["size"][n:] == -7) and np.all(out["desc"][64 * n:] == -7)
    assert np.array_equal(out["xy"][:2 * n].view(np.uint32), ref["xy"].ravel().view(np.uint32))


# ---- the chain of visualOdometry::stereoTriangulate ----
HESSIAN_VO, HESSIAN_SLAM = 500, 1200


@pytest.fixture(scope="module")
def pair():
    """the default synth.Scene at the first pose of the corridor trajectory (the pair of tests/test_gpu_brief.py), 640 x 240"""
    R, t = synth.corridor_trajectory(3, step=0.5)[0]
    left, right, _ = synth.Scene().stereo(R, t, K=K4_SMALL, size=(640, 240))
    assert left.shape == (240, 640, 3)
    return left, right


def gpu_chain(ctx, pair, hessian):
    feats = ctx.surf_extract(list(pair), dict(hessian_threshold=hessian), cap=8192)
    idx, dist = ctx.knn_match(feats[0][6], feats[1][6], k=2, norm=capi.MATCH_L2_F32)
    return feats, ctx.ratio_pairs(idx, dist, feats[0][0], feats[1][0], 0.8)


@pytest.fixture(scope="module")
def chain(pair, ctx):
    return gpu_chain(ctx, pair, HESSIAN_VO)


def test_chain_equals_the_cpu_composition(pair, chain, orc):
    feats, (a, b, mask) = chain
    ref = [restate(im, ("pair", k), HESSIAN_VO) for k, im in enumerate(pair)]
    for k in range(2):
        assert_same(feats[k], ref[k], f"image {k}")
    idx, dist = mn.knn_match(ref[0]["desc"], ref[1]["desc"], 2, mn.L2_F32)
    ca, cb, cmask = mn.ratio_pairs(idx, dist, ref[0]["xy"], ref[1]["xy"], 0.8)
    assert np.array_equal(a, ca) and np.array_equal(b, cb) and np.array_equal(mask, cmask)
    xyz, _ = orc.triangulate(*orc.stereo_projections(*K4_SMALL, synth.KITTI_BASELINE), ca, cb)
    print(f"SURF stereo chain at 640 x 240, threshold {HESSIAN_VO}: {len(ref[0]['xy'])} / {len(ref[1]['xy'])} key points, {len(ca)} "
          f"pairs after the ratio test, {np.mean(np.abs(ca[:, 1] - cb[:, 1]) <= 2):.3f} of them within 2 px of their row, "
          f"{np.mean(xyz[:, 2] > 0):.3f} with positive depth")
    assert len(ca) >= 8   # the one condition on the input


def test_smoke_program_reproduces_the_chain(tmp_path, pair, chain, ctx):
    from test_surf_abi import build_smoke

    _, (a, b, _) = chain
    P1, P2 = capi.stereo_projections(*K4_SMALL, synth.KITTI_BASELINE)
    xyz, _ = ctx.triangulate(P1, P2, a, b)
    _, (sa, sb, _) = gpu_chain(ctx, pair, HESSIAN_SLAM)
    sxyz, _ = ctx.triangulate(P1, P2, sa, sb)
    exe = tmp_path / "surf_stereo_smoke"
    build_smoke(exe)
    files = [str(tmp_path / "left.ppm"), str(tmp_path / "right.ppm")]
    for f, im in zip(files, pair):
        sequence.write_image(f, im)
    run = subprocess.run([str(exe), *files, *(repr(v) for v in K4_SMALL), repr(synth.KITTI_BASELINE), str(HESSIAN_VO),
                          str(HESSIAN_SLAM)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    lines = run.stdout.splitlines()
    heads = [i for i, line in enumerate(lines) if line.startswith("#")]
    assert [lines[i].split()[1] for i in heads] == ["vo", "transform", "reloc", "slam", "surfFeatures"]
    rows = lambda lo, hi: np.array([[float(v) for v in line.split()] for line in lines[lo:hi]], np.float64).reshape(-1, 5).astype(np.float32)   # noqa: E731
    vo, reloc, slam = rows(heads[0] + 1, heads[1]), rows(heads[2] + 1, heads[3]), rows(heads[3] + 1, heads[4])
    assert len(a) >= 8 and int(lines[heads[0]].split()[2]) == len(a) == len(vo)
    assert np.array_equal(vo[:, :2], a) and np.array_equal(vo[:, 2:], xyz, equal_nan=True)
    T = np.array([float(v) for v in lines[heads[1]].split()[2:]], np.float64).reshape(3, 4)
    assert np.array_equal(reloc[:, :2], a) and np.array_equal(reloc[:, 2:], ctx.transform_points(T, xyz), equal_nan=True)
    # the SURF branch of visualSLAM::stereoTriangulate: SURF's pairs (threshold 1200), not ORB's
    assert len(sa) >= 8 and np.array_equal(slam[:, :2], sa) and np.array_equal(slam[:, 2:], sxyz, equal_nan=True)
    assert len(sa) < len(a)
    assert int(lines[heads[4]].split()[2]) == len(chain[0][0][0])
