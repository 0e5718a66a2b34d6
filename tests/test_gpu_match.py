"""svo_knn_match / svo_ratio_pairs on the GPU against tests/match_numpy.py (idx equal, dist equal in its bits), and the
sparse ORB stereo branch end to end: ctx.orb_extract_batch -> knn_match -> ratio_pairs against the oracle's ORB ->
match_numpy, the adaptor's smoke program on the same pair, and the truth check of a rectified pair."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import match_numpy as mn
from ros_stereo_slam_amd import capi, sequence, synth
from test_match_abi import build_smoke

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 7), (63, 65), (1000, 1003), (4097, 6001)]
SMALL = SHAPES[:4]
# dims per norm: every one on the shapes up to 1000 x 1003; on 4097 x 6001 (the restatement walks 24.6 million pairs per
# element) the longest rows -- the 32 KB tile of the float norm --, a row length that takes the 16-byte query loads and one
# that does not
DIMS = {mn.L2_F32: [1, 32, 127, 128, 256], mn.L2_U8: [4, 32, 128, 256], mn.HAMMING: [1, 8, 16]}
DIMS_LARGE = {mn.L2_F32: [32, 127, 256], mn.L2_U8: [32, 256], mn.HAMMING: [8, 1, 16]}


def rows(rng, n, dim, norm):
    if norm == mn.L2_F32:
        return rng.normal(size=(n, dim)).astype(np.float32)
    if norm == mn.L2_U8:
        return rng.integers(0, 256, (n, dim), np.uint8)
    return rng.integers(0, 2**32, (n, dim), np.uint64).astype(np.uint32)


def problem(rng, nq, nt, dim, norm):
    """random rows with a block of train rows duplicated at known positions: row 0 sits at nt // 2 and nt - 1 as well and
    is query 0 too (a three-way tie at distance zero in first and second place); row 1 is repeated at nt // 3 (ties wherever
    it ranks)."""
    q, t = rows(rng, nq, dim, norm), rows(rng, nt, dim, norm)
    if nt >= 7:
        t[nt // 2], t[nt - 1], t[nt // 3] = t[0], t[0], t[1]
        q[0] = t[0]
        if nq > 2:
            q[nq - 1] = t[1]
    return q, t


def same(got, want, what=""):
    gi, gd = (a.cpu().numpy() if hasattr(a, "cpu") else a for a in got)
    assert np.array_equal(gi, want[0]), f"idx differs {what}"
    assert np.array_equal(gd.view(np.uint32), want[1].view(np.uint32)), f"dist bits differ {what}"


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("norm", [mn.L2_F32, mn.L2_U8, mn.HAMMING], ids=["l2_f32", "l2_u8", "hamming"])
def test_knn_equals_the_restatement(ctx, norm, shape):
    nq, nt = shape
    rng = np.random.default_rng(1000 * norm + nq)
    for dim in (DIMS if shape in SMALL else DIMS_LARGE)[norm]:
        q, t = problem(rng, nq, nt, dim, norm)
        idx4, dist4 = mn.select(mn.keys(q, t, norm), 4, norm)   # the k best are the first k of the four best
        if nt >= 7:
            assert list(idx4[0, :3]) == [0, nt // 2, nt - 1] and np.all(dist4[0, :3] == 0)
        for k in (1, 2, 4):
            same(ctx.knn_match(q, t, k=k, norm=norm), (idx4[:, :k], dist4[:, :k]), f"norm {norm} {shape} dim {dim} k {k}")


def test_bytes_equal_floats_on_the_device(ctx):
    rng = np.random.default_rng(2)
    for dim in (32, 256):
        q, t = problem(rng, 300, 401, dim, mn.L2_U8)
        q[1], t[5], t[6] = 0, 255, 0
        a = ctx.knn_match(q, t, k=4, norm=capi.MATCH_L2_U8)
        b = ctx.knn_match(q.astype(np.float32), t.astype(np.float32), k=4, norm=capi.MATCH_L2_F32)
        same(a, b)


def test_sift_sized_problem_on_sampled_queries(ctx):
    """SIFT::create(20000) of src/StereoCV.cpp:65: 20000 x 20000 x 128 floats.  The full restatement is too slow for a
    test; 256 random queries are checked against it."""
    import torch

    rng = np.random.default_rng(20000)
    q, t = problem(rng, 20000, 20000, 128, mn.L2_F32)
    idx, dist = ctx.knn_match(torch.from_numpy(q).cuda(), torch.from_numpy(t).cuda(), k=2, norm=capi.MATCH_L2_F32)
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
    sel = np.sort(np.r_[0, 19999, rng.choice(np.arange(1, 19999), 254, replace=False)])
    same((idx[sel], dist[sel]), mn.knn_match(q[sel], t, 2, mn.L2_F32))
    assert idx.min() >= 0 and idx.max() < 20000 and np.all(dist[:, 0] <= dist[:, 1])


@pytest.mark.parametrize("norm,dim", [(mn.L2_U8, 32), (mn.L2_F32, 127), (mn.HAMMING, 8)], ids=["l2_u8", "l2_f32", "hamming"])
def test_batch_of_sixteen_equals_one_call_each(ctx, norm, dim):
    rng = np.random.default_rng(16 + norm)
    nqs = [300, 0, 1, 257, 1000, 64, 65, 511, 5, 256, 90, 700, 33, 2, 128, 401]
    nts = [500, 40, 1, 1, 1003, 0, 2, 3, 4097, 31, 32, 33, 640, 7, 1, 256]   # an empty range, ranges of one row
    assert len(nqs) == len(nts) == 16
    qo, to = np.r_[0, np.cumsum(nqs)].astype(np.int32), np.r_[0, np.cumsum(nts)].astype(np.int32)
    q, t = rows(rng, qo[-1], dim, norm), rows(rng, to[-1], dim, norm)
    t[to[4] + 9], t[to[4] + 500] = t[to[4] + 3], t[to[4] + 3]
    q[qo[4]] = t[to[4] + 3]
    for k in (2, 4):
        got = ctx.knn_match(q, t, k=k, norm=norm, q_offsets=qo, t_offsets=to)
        same(got, mn.knn_match_batch(q, t, qo, to, k, norm), "batch against the restatement")
        for p in range(16):
            one = ctx.knn_match(q[qo[p]:qo[p + 1]], t[to[p]:to[p + 1]], k=k, norm=norm)
            same((got[0][qo[p]:qo[p + 1]], got[1][qo[p]:qo[p + 1]]), one, f"problem {p}")
    assert np.all(got[0][qo[5]:qo[6]] == -1) and np.all(np.isinf(got[1][qo[5]:qo[6]]))      # no train rows
    assert np.all(got[0][qo[2]:qo[3], 1:] == -1) and np.all(got[0][qo[2]:qo[3], 0] == 0)     # one train row


def test_host_mode_equals_device_mode(ctx):
    import torch

    rng = np.random.default_rng(7)
    for norm, dim in ((mn.L2_F32, 128), (mn.L2_F32, 5), (mn.L2_U8, 32), (mn.HAMMING, 8)):
        q, t = problem(rng, 777, 1500, dim, norm)
        qo, to = np.array([0, 300, 777], np.int32), np.array([0, 1, 1500], np.int32)
        host = ctx.knn_match(q, t, k=4, norm=norm, q_offsets=qo, t_offsets=to)
        qt = torch.from_numpy(q.view(np.int32) if norm == mn.HAMMING else q).cuda()
        tt = torch.from_numpy(t.view(np.int32) if norm == mn.HAMMING else t).cuda()
        dev = ctx.knn_match(qt, tt, k=4, norm=norm, q_offsets=qo, t_offsets=to)
        assert dev[0].is_cuda and dev[1].is_cuda
        same(dev, host)
        same(host, mn.knn_match_batch(q, t, qo, to, 4, norm))


def raw_knn(ctx, norm, q, t, dim, qo, to, nprob, k, idx, dist, mem=capi.MEM_HOST):
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    return ctx.lib.svo_knn_match(ctx._h, norm, p(q), p(t), dim, p(qo), p(to), nprob, k, p(idx), p(dist), mem)


def test_refusals(ctx):
    q, t = np.zeros((4, 32), np.float32), np.zeros((5, 32), np.float32)
    qo, to = np.array([0, 4], np.int32), np.array([0, 5], np.int32)
    idx, dist = np.zeros((4, 2), np.int32), np.zeros((4, 2), np.float32)
    ok = lambda **kw: raw_knn(ctx, **{**dict(norm=0, q=q, t=t, dim=32, qo=qo, to=to, nprob=1, k=2, idx=idx, dist=dist), **kw})
    assert ok() == capi.SVO_OK
    assert ok(norm=3) == capi.SVO_ERR_ARG and ok(norm=-1) == capi.SVO_ERR_ARG
    assert ok(dim=0) == capi.SVO_ERR_ARG and ok(dim=257) == capi.SVO_ERR_ARG
    assert ok(norm=1, dim=6) == capi.SVO_ERR_ARG and ok(norm=1, dim=0) == capi.SVO_ERR_ARG and ok(norm=1, dim=260) == capi.SVO_ERR_ARG
    assert ok(norm=2, dim=17) == capi.SVO_ERR_ARG and ok(norm=2, dim=0) == capi.SVO_ERR_ARG
    assert ok(k=0) == capi.SVO_ERR_ARG and ok(k=5) == capi.SVO_ERR_ARG
    assert ok(nprob=0) == capi.SVO_ERR_ARG and ok(nprob=17) == capi.SVO_ERR_ARG
    assert ok(qo=np.array([4, 0], np.int32)) == capi.SVO_ERR_ARG and ok(to=np.array([5, 2], np.int32)) == capi.SVO_ERR_ARG
    assert ok(qo=None) == capi.SVO_ERR_ARG and ok(to=None) == capi.SVO_ERR_ARG
    assert ok(q=None) == capi.SVO_ERR_ARG and ok(t=None) == capi.SVO_ERR_ARG
    assert ok(idx=None) == capi.SVO_ERR_ARG and ok(dist=None) == capi.SVO_ERR_ARG
    assert ok(mem=2) == capi.SVO_ERR_ARG
    # rows are read as 32-bit words: a pointer one byte off is refused
    raw = np.zeros(5 * 32 * 4 + 4, np.uint8)
    off = raw[1:1 + 5 * 32 * 4].view(np.float32).reshape(5, 32)
    assert off.ctypes.data % 4 == 1
    assert ok(q=off[:4]) == capi.SVO_ERR_ARG and ok(t=off) == capi.SVO_ERR_ARG
    # capacity: 32768 rows per problem are accepted by the argument checks, 32769 are not (nothing is read: dim 1)
    big = np.zeros((32769, 1), np.float32)
    bi, bd = np.zeros((32769, 1), np.int32), np.zeros((32769, 1), np.float32)
    over, one = np.array([0, 32769], np.int32), np.array([0, 1], np.int32)
    assert raw_knn(ctx, 0, big, big, 1, over, one, 1, 1, bi, bd) == capi.SVO_ERR_CAPACITY
    assert raw_knn(ctx, 0, big, big, 1, one, over, 1, 1, bi, bd) == capi.SVO_ERR_CAPACITY
    two = np.array([0, 32768, 32769], np.int32)
    assert raw_knn(ctx, 0, big, big, 1, two, np.array([0, 1, 2], np.int32), 2, 1, bi, bd) == capi.SVO_OK
    with pytest.raises(capi.SvoError) as e:
        ctx.knn_match(big, big[:1], k=1, norm=capi.MATCH_L2_F32)
    assert e.value.code == capi.SVO_ERR_CAPACITY
    # svo_ratio_pairs
    cnt = C.c_int(-5)
    xy = np.zeros((5, 2), np.float32)
    o1, o2 = xy.copy(), xy.copy()
    rp = lambda i, d, n, k, c: ctx.lib.svo_ratio_pairs(ctx._h, capi._ptr(i), capi._ptr(d), n, k, C.c_double(0.8), capi._ptr(xy),
                                                       capi._ptr(xy), capi._ptr(o1), capi._ptr(o2), None, c, capi.MEM_HOST)
    assert rp(idx, dist, 4, 2, None) == capi.SVO_ERR_ARG
    assert rp(None, dist, 4, 2, C.byref(cnt)) == capi.SVO_ERR_ARG and rp(idx, dist, 4, 5, C.byref(cnt)) == capi.SVO_ERR_ARG
    assert rp(idx, dist, -1, 2, C.byref(cnt)) == capi.SVO_ERR_ARG
    assert rp(idx, dist, 0, 2, C.byref(cnt)) == capi.SVO_OK and cnt.value == 0


def test_nan_and_infinite_keys_order_last(ctx):
    """include/svo.h: a NaN key orders behind every number (+inf included); its dist is NaN."""
    rng = np.random.default_rng(3)
    q, t = rng.normal(size=(70, 9)).astype(np.float32), rng.normal(size=(4, 9)).astype(np.float32)
    t[1, 4], t[2, 0] = np.nan, np.inf
    want = mn.knn_match(q, t, 4, mn.L2_F32)
    idx, dist = ctx.knn_match(q, t, k=4, norm=capi.MATCH_L2_F32)
    assert np.array_equal(idx, want[0]) and np.all(idx[:, 2] == 2) and np.all(idx[:, 3] == 1)
    assert np.array_equal(dist[:, :3].view(np.uint32), want[1][:, :3].view(np.uint32))
    assert np.all(np.isinf(dist[:, 2])) and np.all(np.isnan(dist[:, 3])) and np.all(np.isnan(want[1][:, 3]))
    idx2, dist2 = ctx.knn_match(q, t, k=2, norm=capi.MATCH_L2_F32)
    assert np.array_equal(idx2, idx[:, :2]) and np.all(np.isfinite(dist2))


@pytest.mark.parametrize("ratio", [0.6, 0.8, 1.0])
def test_ratio_pairs_equals_the_restatement(ctx, ratio):
    import torch

    rng = np.random.default_rng(11)
    cases = []
    for norm, dim, nq, nt, k in ((mn.L2_U8, 32, 1000, 1003, 2), (mn.L2_F32, 32, 4097, 6001, 4), (mn.HAMMING, 8, 63, 65, 2),
                                 (mn.L2_U8, 32, 50, 1, 2), (mn.L2_U8, 32, 50, 30, 1), (mn.L2_F32, 1, 1, 7, 2)):
        q, t = problem(rng, nq, nt, dim, norm)
        if norm == mn.L2_U8 and nt > 800:    # planted first and second neighbours, so that the three ratios cut differently
            t[100:400] = np.clip(q[100:400].astype(int) + rng.integers(-3, 4, (300, dim)), 0, 255)
            t[500:600] = np.clip(q[100:200].astype(int) + rng.integers(-4, 5, (100, dim)), 0, 255)    # d0 / d1 near 0.8
            t[600:800] = np.clip(q[200:400].astype(int) + rng.integers(-8, 9, (200, dim)), 0, 255)    # near 0.4
        cases.append(ctx.knn_match(q, t, k=k, norm=norm) + (nq, nt))
    # the edge of the double comparison: 4 < 0.8 * 5 is false in double
    below, above = np.nextafter(np.float32(4), np.float32(0)), np.nextafter(np.float32(5), np.float32(6))
    cases.append((np.array([[0, 1]] * 4 + [[1, -1]], np.int32),
                  np.array([[4, 5], [below, 5], [4, above], [5, 5], [0, np.inf]], np.float32), 5, 2))
    kept = 0
    for idx, dist, nq, nt in cases:
        xq, xt = rng.uniform(0, 1241, (nq, 2)).astype(np.float32), rng.uniform(0, 1241, (nt, 2)).astype(np.float32)
        want = mn.ratio_pairs(idx, dist, xq, xt, ratio)
        got = ctx.ratio_pairs(idx, dist, xq, xt, ratio)
        for g, w in zip(got, want):
            assert np.array_equal(g, w)
        dev = ctx.ratio_pairs(*(torch.from_numpy(a).cuda() for a in (idx, dist, xq, xt)), ratio)
        for g, w in zip(dev, want):
            assert g.is_cuda and np.array_equal(g.cpu().numpy(), w)
        kept += len(want[0])
    assert kept > 100
    if ratio == 0.8:
        assert list(got[2]) == [0, 1, 1, 0, 0]   # the last case: the edge, a tie, an empty second slot


# ---- the sparse stereo branch, end to end ---------------------------------------------------------------------------
N_FEATURES = 1000          # ORB::create(1000), src/triangulation.cpp:105
TRUTH_PAIRS = 240          # measured on the CPU side alone (oracle ORB -> match_numpy), see test_truth_of_a_rectified_pair
TRUTH_WITHIN = 211
TRUTH_DY = 2.0


@pytest.fixture(scope="module")
def pair():
    """the default synth.Scene at the first pose of the corridor trajectory, KITTI intrinsics, 1241 x 376"""
    R, t = synth.corridor_trajectory(3, step=0.5)[0]
    left, right, _ = synth.Scene().stereo(R, t)
    assert left.shape == (376, 1241, 3)
    return left, right


def u8(desc):
    return np.ascontiguousarray(desc).view(np.uint8).reshape(len(desc), 32)


@pytest.fixture(scope="module")
def cpu_side(pair, orc):
    a, b = (orc.orb_extract_cv(im, N_FEATURES) for im in pair)
    idx, dist = mn.knn_match(u8(a[5]), u8(b[5]), 2, mn.L2_U8)     # desc.convertTo(CV_32F) + BFMatcher (L2)
    return a, b, idx, dist, mn.ratio_pairs(idx, dist, a[0], b[0], 0.8)


@pytest.fixture(scope="module")
def gpu_side(pair, ctx):
    a, b = ctx.orb_extract_batch(list(pair), n_features=N_FEATURES)
    idx, dist = ctx.knn_match(a[4], b[4], k=2, norm=capi.MATCH_L2_U8)   # the byte view of the descriptor words
    return a, b, idx, dist, ctx.ratio_pairs(idx, dist, a[0], b[0], 0.8)


def test_end_to_end_equals_the_cpu_composition(cpu_side, gpu_side):
    ca, cb, cidx, cdist, cpairs = cpu_side
    ga, gb, gidx, gdist, gpairs = gpu_side
    assert np.array_equal(ga[0], ca[0]) and np.array_equal(gb[0], cb[0])          # rests on tests/test_gpu_orb.py
    assert np.array_equal(ga[4], ca[5]) and np.array_equal(gb[4], cb[5])
    same((gidx, gdist), (cidx, cdist))
    for g, c in zip(gpairs, cpairs):
        assert np.array_equal(g, c)
    assert len(gpairs[0]) >= 100


def test_truth_of_a_rectified_pair(cpu_side, gpu_side):
    """Every true match of a rectified pair has y1 == y2.  Measured on the CPU side alone (the oracle's ORB with 1000
    features on both images of the default scene's first pose, match_numpy, ratio 0.8): 240 of 1000 queries survive the ratio
    test and 211 of them (87.9 %) have |y1 - y2| <= 2 px (193 within 1 px, 228 within 3 px).  The GPU pair list must equal the
    CPU one, so it is held to exactly those figures."""
    for p1, p2, mask in (cpu_side[4], gpu_side[4]):
        dy = np.abs(p1[:, 1] - p2[:, 1])
        print(f"pairs {len(p1)} of {len(mask)}, |dy| <= {TRUTH_DY}: {(dy <= TRUTH_DY).sum()}")
        assert len(p1) == TRUTH_PAIRS and int(mask.sum()) == TRUTH_PAIRS
        assert int((dy <= TRUTH_DY).sum()) == TRUTH_WITHIN


def test_smoke_program_reproduces_the_composition(tmp_path, pair, gpu_side, orc):
    exe = tmp_path / "sparse_triangulate_smoke"
    build_smoke(exe)
    files = [str(tmp_path / "left.ppm"), str(tmp_path / "right.ppm")]
    for f, im in zip(files, pair):
        sequence.write_image(f, im)
    run = subprocess.run([str(exe), *files], check=True, capture_output=True, text=True, timeout=120)
    got = np.array([[float(v) for v in line.split()] for line in run.stdout.splitlines() if not line.startswith("#")],
                   np.float64).reshape(-1, 8).astype(np.float32)
    p1, p2, _ = gpu_side[4]
    assert np.array_equal(got[:, :2], p1)                                   # the 2-D points, exactly
    # svo_triangulate / svo_get_colors are bit for bit with the oracle (tests/test_gpu_geometry.py, test_gpu_colour.py)
    P1, P2 = orc.stereo_projections(*synth.KITTI_K, synth.KITTI_BASELINE)
    xyz, _ = orc.triangulate(P1, P2, p1, p2)
    assert np.array_equal(got[:, 2:5], xyz, equal_nan=True)
    assert np.array_equal(got[:, 5:8], orc.get_colors(pair[0], p1))
