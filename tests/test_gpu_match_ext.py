"""svo_match_cross, svo_radius_match and svo_knn_match_gated on the GPU against tests/match_ext_numpy.py: idx equal, dist equal in
its bits, row offsets equal.  Sizes sit at the seams of csrc/match_plan.hip.h (MT 32 train rows a tile, MQ 256 queries a
workgroup, the split of a long train range over workgroups), ties meet across a tile and across a split, outputs lie behind guard
bands in both memories, batches equal their problems, and svo_knn_match / svo_ratio_pairs are undisturbed."""
import ctypes as C
import pathlib
import re

import numpy as np
import pytest

import match_ext_numpy as mx
import match_numpy as mn
from ros_stereo_slam_amd import capi

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parents[1]
PLAN = (ROOT / "ros_stereo_slam_amd" / "csrc" / "match_plan.hip.h").read_text()
MT, MQ, MAX_SPLIT = (int(re.search(rf"constexpr int {n} = (\d+);", PLAN).group(1)) for n in ("MT", "MQ", "MAX_SPLIT"))
NQS, NTS = [0, 1, MQ - 1, MQ, MQ + 1], [0, 1, MT - 1, MT, MT + 1, 2 * MT + 1]
SPLIT_CASE = (3, 2 * MT * MAX_SPLIT // 2 + 1)   # 3 x 2049: one query block, 65 tiles over 64 workgroups
SHAPES = [(q, t) for q in NQS for t in NTS] + [SPLIT_CASE]
# the least and the largest dim of each norm, and one whose rows are no multiple of four 32-bit words
DIMS = {mn.L2_F32: [1, 6, 256], mn.L2_U8: [4, 20, 256], mn.HAMMING: [1, 6, 16]}
NORMS = pytest.mark.parametrize("norm", [mn.L2_F32, mn.L2_U8, mn.HAMMING], ids=["l2_f32", "l2_u8", "hamming"])
SENTINEL_I, SENTINEL_F = -77, -7.5


def test_the_seams_are_the_kernels():
    assert (MT, MQ, MAX_SPLIT) == (32, 256, 64) and SPLIT_CASE == (3, 2049)
    assert f"#define SVO_RADIUS_MAX_PER_QUERY {mx.MAX_PER_QUERY}" in (ROOT / "include" / "svo.h").read_text()
    assert capi.RADIUS_MAX_PER_QUERY == mx.MAX_PER_QUERY and (capi.CROSS_MUTUAL, capi.CROSS_CV) == (mx.MUTUAL, mx.CV)


def rows(rng, n, dim, norm):
    if norm == mn.L2_F32:
        return rng.integers(-3, 4, (n, dim)).astype(np.float32) if dim < 4 else rng.normal(size=(n, dim)).astype(np.float32)
    if norm == mn.L2_U8:
        return rng.integers(0, 256, (n, dim), np.uint8)
    return rng.integers(0, 2**32, (n, dim), np.uint64).astype(np.uint32)


def problem(rng, nq, nt, dim, norm):
    """random rows with duplicates on both sides: train row 0 again at MT - 1, MT (a tile seam), 2 * MT - 1 and 2 * MT (the seam of
    two workgroups when the range is split in pairs of tiles) and at the end; query 0 and the last query equal it, query 1 is
    repeated as query 2."""
    q, t = rows(rng, nq, dim, norm), rows(rng, nt, dim, norm)
    for r in (MT - 1, MT, 2 * MT - 1, 2 * MT, nt - 1):
        if 0 < r < nt:
            t[r] = t[0]
    if nq and nt:
        q[0] = q[nq - 1] = t[0]
    if nq > 2:
        q[2] = q[1]
    return q, t


def lattice(rng, n):
    """key points on a lattice of quarter pixels: the gate's boundaries are met exactly"""
    return (rng.integers(0, 160, (n, 2)) * 0.25).astype(np.float32)


def cases(norm, seed):
    rng = np.random.default_rng(seed)
    for n, (nq, nt) in enumerate(SHAPES):
        for dim in (DIMS[norm] if (nq, nt) == SPLIT_CASE else [DIMS[norm][n % 3]]):
            q, t = problem(rng, nq, nt, dim, norm)
            yield q, t, mn.keys(q, t, norm), f"norm {norm} {nq} x {nt} dim {dim}"


def same(got, want, what=""):
    gi, gd = (a.cpu().numpy() if hasattr(a, "cpu") else a for a in got)
    assert np.array_equal(gi, want[0]), f"idx differs: {what}"
    assert np.array_equal(gd.view(np.uint32), np.asarray(want[1], np.float32).view(np.uint32)), f"dist bits differ: {what}"


def same_csr(got, want, what=""):
    off = got[0].cpu().numpy() if hasattr(got[0], "cpu") else got[0]
    assert np.array_equal(off.astype(np.int64), want[0]), f"row offsets differ: {what}"
    same(got[1:], want[1:], what)


@NORMS
def test_cross_equals_the_restatement(ctx, norm):
    differ = 0
    for q, t, key, what in cases(norm, 100 + norm):
        want = [mx.cross_from_keys(key, norm, m) for m in (mx.MUTUAL, mx.CV)]
        for mode in (mx.MUTUAL, mx.CV):
            same(ctx.match_cross(q, t, norm=norm, mode=mode), want[mode], f"{what} mode {mode}")
        differ += int(np.sum((want[mx.CV][0] >= 0) & (want[mx.MUTUAL][0] < 0)))
        assert np.all((want[mx.MUTUAL][0] < 0) | (want[mx.MUTUAL][0] == want[mx.CV][0])), what
    assert differ > 0, "no case pairs a query in CV alone"


def some_radius(key, norm, rng):
    """a returned float that occurs, so that the boundary dist == max_distance is met"""
    d = mx.root(key, norm).ravel()
    d = d[np.isfinite(d)]
    return float(np.sort(d)[len(d) // 5]) if len(d) else 1.0


@NORMS
def test_radius_equals_the_restatement(ctx, norm):
    rng = np.random.default_rng(200 + norm)
    nonempty = 0
    for q, t, key, what in cases(norm, 200 + norm):
        for r in (0.0, some_radius(key, norm, rng), np.inf):
            want = mx.radius_from_keys(key, norm, r)
            total = int(want[0][-1])
            same_csr(ctx.radius_match(q, t, r, norm=norm), want, f"{what} radius {r}")
            same_csr(ctx.radius_match(q, t, r, norm=norm, capacity=total), want, f"{what} radius {r}, capacity met")
            if r == np.inf:
                assert total == key.shape[0] * key.shape[1]              # takes every row
            if total > 0:
                nonempty += 1
                with pytest.raises(capi.SvoError) as e:
                    ctx.radius_match(q, t, r, norm=norm, capacity=total - 1)
                assert e.value.code == capi.SVO_ERR_CAPACITY and e.value.total == total
                assert np.array_equal(e.value.row_offsets.astype(np.int64), want[0])   # the needed counts
    assert nonempty > 50


def test_radius_with_more_queries_than_one_chunk_of_the_row_scan(ctx):
    """1025 queries against 8 train rows: the scan of the rows' counts (1024 a chunk) takes a second chunk, whose one row starts at
    the first chunk's carry.  Train row j is (10 j, 0, 0, 0), query i is (x_i, 0, 0, 0), the radius 12: a row has 0 ... 3 matches."""
    rng = np.random.default_rng(300)
    t = np.zeros((8, 4), np.uint8)
    t[:, 0] = 10 * np.arange(8)
    q = np.zeros((1025, 4), np.uint8)
    q[:, 0] = rng.integers(0, 256, 1025)
    q[-1, 0] = 40                                                   # the row of the second chunk has matches of its own
    want = mx.radius_match(q, t, 12.0, norm=mn.L2_U8)
    counts = np.diff(want[0])
    assert counts.min() == 0 and counts.max() == 3 and set(counts) == {0, 1, 2, 3} and want[0][1024] > 0 and counts[1024] == 3
    same_csr(ctx.radius_match(q, t, 12.0, norm=mn.L2_U8), want, "1025 x 8")


@NORMS
def test_gated_equals_the_restatement(ctx, norm):
    rng = np.random.default_rng(300 + norm)
    short = 0
    for q, t, key, what in cases(norm, 300 + norm):
        nq, nt = key.shape
        k = 1 + (nq + nt) % 4
        plain = ctx.knn_match(q, t, k=k, norm=norm)
        same(ctx.knn_match_gated(q, t, k=k, norm=norm, mask=np.ones((nq, nt), np.uint8)), plain, f"{what}: all ones")
        none = ctx.knn_match_gated(q, t, k=k, norm=norm, mask=np.zeros((nq, nt), np.uint8))
        assert np.all(none[0] == -1) and np.all(np.isinf(none[1])), f"{what}: all zero"
        mask = (rng.random((nq, nt)) < 0.08).astype(np.uint8) * rng.integers(1, 256, (nq, nt)).astype(np.uint8)
        if nq > 3 and nt > 3:
            mask[1], mask[2, :], mask[3] = 0, 0, 255          # 0 candidates, then exactly one, then all
            mask[2, nt - 1] = 1
        want = mx.masked_from_keys(key, mask, k, norm)
        same(ctx.knn_match_gated(q, t, k=k, norm=norm, mask=mask), want, f"{what}: random mask")
        short += int(np.sum(want[0] < 0))
        # a rectified pair's band: rows on a lattice of quarter pixels, so that the boundaries are met exactly
        xq, xt = lattice(rng, nq), lattice(rng, nt)
        gate = (2.0, 0.0, 12.5)
        gm = mx.gate_mask(xq, xt, gate)
        got = ctx.knn_match_gated(q, t, k=k, norm=norm, gate=gate, xy_query=xq, xy_train=xt)
        same(got, mx.masked_from_keys(key, gm, k, norm), f"{what}: gate against the restatement")
        same(got, ctx.knn_match_gated(q, t, k=k, norm=norm, mask=gm), f"{what}: gate against its byte mask")
        if nq and nt:
            dy, dx = np.abs(xq[:, None, 1] - xt[None, :, 1]), xq[:, None, 0] - xt[None, :, 0]
            short += int((dy == 2.0).any() and (dx == 0.0).any())
    assert short > 100


def test_nan_rows(ctx):
    rng = np.random.default_rng(5)
    q, t = rng.normal(size=(70, 9)).astype(np.float32), rng.normal(size=(40, 9)).astype(np.float32)
    t[1, 4], t[2, 0], q[3, 1], q[4, 2] = np.nan, np.inf, np.nan, np.inf
    key = mn.keys(q, t, mn.L2_F32)
    for mode in (mx.MUTUAL, mx.CV):
        same(ctx.match_cross(q, t, norm=mn.L2_F32, mode=mode), mx.cross_from_keys(key, mn.L2_F32, mode), f"mode {mode}")
    for r in (1.0, 4.0, np.inf):
        want = mx.radius_from_keys(key, mn.L2_F32, r)
        same_csr(ctx.radius_match(q, t, r, norm=mn.L2_F32), want)
        assert not np.isnan(want[2]).any() and want[0][4] == want[0][3]        # a NaN never passes: query 3 has no match
    assert int(mx.radius_from_keys(key, mn.L2_F32, np.inf)[0][-1]) == int(np.sum(~np.isnan(key))) < key.size   # +inf passes, NaN not
    with pytest.raises(capi.SvoError) as e:
        ctx.radius_match(q, t, np.nan, norm=mn.L2_F32)
    assert e.value.code == capi.SVO_ERR_ARG
    assert int(ctx.radius_match(q, t, -1.0, norm=mn.L2_F32)[0][-1]) == 0


def test_two_integer_keys_with_one_rooted_float(ctx):
    """two neighbouring integer keys above 16000000 root to the same float: both pass a radius equal to it, in key order; the next float below
    admits neither (M1 / M6)"""
    k0 = next(k for k in range(16000001, 16000100) if np.sqrt(np.float32(k)) == np.sqrt(np.float32(k + 1)))
    assert k0 + 1 <= 250 * 255 * 255
    def row(key):                                    # a byte row whose squared distance to zero is `key`
        out, left = [], key
        while left > 0:
            v = min(255, int(np.sqrt(left)))
            out.append(v)
            left -= v * v
        return out
    a, b = row(k0 + 1), row(k0)
    dim = 256
    assert max(len(a), len(b)) <= dim
    t = np.zeros((3, dim), np.uint8)
    t[0, :len(a)], t[1, :len(b)] = a, b
    t[2, :] = 255
    q = np.zeros((1, dim), np.uint8)
    key = mn.keys(q, t, mn.L2_U8)
    assert list(key[0, :2]) == [k0 + 1, k0]
    r = float(np.sqrt(np.float32(k0)))
    want = mx.radius_from_keys(key, mn.L2_U8, r)
    assert list(want[1]) == [1, 0]
    same_csr(ctx.radius_match(q, t, r, norm=mn.L2_U8), want)
    below = float(np.nextafter(np.float32(r), np.float32(0)))
    same_csr(ctx.radius_match(q, t, below, norm=mn.L2_U8), mx.radius_from_keys(key, mn.L2_U8, below))
    assert int(mx.radius_from_keys(key, mn.L2_U8, below)[0][-1]) == 0


def test_a_query_past_the_per_query_bound(ctx):
    t = np.zeros((mx.MAX_PER_QUERY + 1, 1), np.uint32)
    q = np.zeros((2, 1), np.uint32)
    q[1] = 1
    off, idx, dist = ctx.radius_match(q, t[:-1], 0.0, norm=mn.HAMMING)
    assert list(off) == [0, mx.MAX_PER_QUERY, mx.MAX_PER_QUERY] and np.array_equal(idx, np.arange(mx.MAX_PER_QUERY)) and not dist.any()
    with pytest.raises(capi.SvoError) as e:
        ctx.radius_match(q, t, 0.0, norm=mn.HAMMING)
    assert e.value.code == capi.SVO_ERR_CAPACITY and list(e.value.row_offsets) == [0, mx.MAX_PER_QUERY + 1, mx.MAX_PER_QUERY + 1]
    assert mx.radius_verdict(np.array([0, mx.MAX_PER_QUERY + 1, mx.MAX_PER_QUERY + 1]), 10**6) == "capacity"
    off, idx, dist = ctx.radius_match(q, t, 1.0, norm=mn.HAMMING, q_offsets=[0, 0, 2], t_offsets=[0, 5, 100])   # both rows, sorted
    assert list(off) == [0, 0, 95, 190] and np.array_equal(idx[95:], np.arange(95)) and np.all(dist[:95] == 0) and np.all(dist[95:] == 1)


BATCH_NQ = [300, 0, 1, 257, 40, 64, 65, 511, 5, 256, 90, 70, 33, 2, 128, 3]
BATCH_NT = [100, 40, 1, 1, 1003, 0, 2, 3, 2049, 31, 32, 33, 640, 7, 1, 256]


@NORMS
def test_batch_of_sixteen_equals_one_call_each(ctx, norm):
    rng = np.random.default_rng(16 + norm)
    dim = DIMS[norm][1]
    qo, to = np.r_[0, np.cumsum(BATCH_NQ)].astype(np.int32), np.r_[0, np.cumsum(BATCH_NT)].astype(np.int32)
    q, t = rows(rng, qo[-1], dim, norm), rows(rng, to[-1], dim, norm)
    t[to[4] + 9], t[to[4] + 500] = t[to[4] + 3], t[to[4] + 3]
    q[qo[4]] = t[to[4] + 3]
    kk = mx.batch(lambda a, b, p: mn.keys(a, b, norm), q, t, qo, to)
    r = some_radius(np.concatenate([k.ravel() for k in kk]).reshape(1, -1), norm, rng)
    xq, xt = lattice(rng, qo[-1]), lattice(rng, to[-1])
    gate = (1.0, -3.0, 20.0)
    masks = [(rng.random(k.shape) < 0.2).astype(np.uint8) for k in kk]
    flat = np.concatenate([m.ravel() for m in masks])
    cross = {m: ctx.match_cross(q, t, norm=norm, mode=m, q_offsets=qo, t_offsets=to) for m in (mx.MUTUAL, mx.CV)}
    off, ridx, rdist = ctx.radius_match(q, t, r, norm=norm, q_offsets=qo, t_offsets=to)
    byte = ctx.knn_match_gated(q, t, k=3, norm=norm, mask=flat, q_offsets=qo, t_offsets=to)
    band = ctx.knn_match_gated(q, t, k=3, norm=norm, gate=gate, xy_query=xq, xy_train=xt, q_offsets=qo, t_offsets=to)
    for p in range(16):
        a, b, qs, ts = int(qo[p]), int(qo[p + 1]), q[qo[p]:qo[p + 1]], t[to[p]:to[p + 1]]
        for m in (mx.MUTUAL, mx.CV):
            part = (cross[m][0][a:b], cross[m][1][a:b])
            same(part, mx.cross_from_keys(kk[p], norm, m), f"cross {m}, problem {p}")
            same(part, ctx.match_cross(qs, ts, norm=norm, mode=m), f"cross {m}, problem {p} on its own")
        o = off[a + p:b + p + 1].astype(np.int64)
        part = (o - o[0], ridx[o[0]:o[-1]], rdist[o[0]:o[-1]])
        same_csr(part, mx.radius_from_keys(kk[p], norm, r), f"radius, problem {p}")
        same_csr(part, ctx.radius_match(qs, ts, r, norm=norm), f"radius, problem {p} on its own")
        assert p == 0 or o[0] == off[a + p - 1]
        same((byte[0][a:b], byte[1][a:b]), mx.masked_from_keys(kk[p], masks[p], 3, norm), f"mask, problem {p}")
        same((byte[0][a:b], byte[1][a:b]), ctx.knn_match_gated(qs, ts, k=3, norm=norm, mask=masks[p]), f"mask, problem {p} alone")
        gm = mx.gate_mask(xq[a:b], xt[to[p]:to[p + 1]], gate)
        same((band[0][a:b], band[1][a:b]), mx.masked_from_keys(kk[p], gm, 3, norm), f"gate, problem {p}")
        same((band[0][a:b], band[1][a:b]),
             ctx.knn_match_gated(qs, ts, k=3, norm=norm, gate=gate, xy_query=xq[a:b], xy_train=xt[to[p]:to[p + 1]]), f"gate, problem {p} alone")


def guarded(n, dtype, device):
    """n elements between two bands of 64 sentinels -> (whole buffer, pointer of the inner part, reader of the whole)"""
    fill = SENTINEL_I if np.issubdtype(dtype, np.integer) else SENTINEL_F
    host = np.full(n + 128, fill, dtype)
    if not device:
        return host, C.c_void_p(host.ctypes.data + 64 * host.itemsize), lambda: host
    import torch

    dev = torch.from_numpy(host).cuda()
    return dev, C.c_void_p(dev.data_ptr() + 64 * host.itemsize), lambda: dev.cpu().numpy()


def inner(read, n, what):
    a = read()
    fill = SENTINEL_I if np.issubdtype(a.dtype, np.integer) else SENTINEL_F
    assert np.all(a[:64] == fill) and np.all(a[64 + n:] == fill), f"{what}: a guard band was written"
    return a[64:64 + n]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_outputs_behind_guard_bands(ctx, device):
    """the raw entry points on inputs and outputs that end where the next allocation's sentinels begin"""
    rng = np.random.default_rng(9)
    norm, dim, nq, nt = mn.L2_U8, 20, MQ + 1, 2 * MT + 1
    q, t = problem(rng, nq, nt, dim, norm)
    key = mn.keys(q, t, norm)
    xq, xt = lattice(rng, nq), lattice(rng, nt)
    mask = (rng.random((nq, nt)) < 0.1).astype(np.uint8)
    qo, to = np.array([0, nq], np.int32), np.array([0, nt], np.int32)
    mem = capi.MEM_DEVICE if device else capi.MEM_HOST
    if device:
        import torch

        keep = [torch.from_numpy(a).cuda() for a in (q, t, xq, xt, mask)]
        pq, pt, pxq, pxt, pm = (C.c_void_p(a.data_ptr()) for a in keep)
    else:
        pq, pt, pxq, pxt, pm = (capi._ptr(a) for a in (q, t, xq, xt, mask))
    lib, h, p = ctx.lib, ctx._h, capi._ptr
    for mode in (mx.MUTUAL, mx.CV):
        (_, pi, ri), (_, pd, rd) = guarded(nq, np.int32, device), guarded(nq, np.float32, device)
        assert lib.svo_match_cross(h, norm, pq, pt, dim, p(qo), p(to), 1, mode, pi, pd, mem) == 0
        ctx.sync()
        same((inner(ri, nq, "cross idx"), inner(rd, nq, "cross dist")), mx.cross_from_keys(key, norm, mode))
    r = some_radius(key, norm, rng)
    want = mx.radius_from_keys(key, norm, r)
    total = int(want[0][-1])
    for cap in (total, total - 1):
        (_, po, ro), (_, pi, ri), (_, pd, rd) = guarded(nq + 1, np.int32, device), guarded(cap, np.int32, device), guarded(cap, np.float32, device)
        n = C.c_int(-1)
        rc = lib.svo_radius_match(h, norm, pq, pt, dim, p(qo), p(to), 1, C.c_float(r), po, pi, pd, cap, C.byref(n), mem)
        ctx.sync()
        assert n.value == total and np.array_equal(inner(ro, nq + 1, "radius offsets"), want[0])
        if cap == total:
            assert rc == 0
            same((inner(ri, cap, "radius idx"), inner(rd, cap, "radius dist")), want[1:])
        else:
            assert rc == capi.SVO_ERR_CAPACITY     # one short: the offsets, and nothing else
            assert np.all(inner(ri, cap, "radius idx") == SENTINEL_I) and np.all(inner(rd, cap, "radius dist") == SENTINEL_F)
    g = capi.MatchGate(2.0, 0.0, 12.5)
    for form in ("mask", "gate"):
        (_, pi, ri), (_, pd, rd) = guarded(nq * 2, np.int32, device), guarded(nq * 2, np.float32, device)
        args = (pm, None, None, None) if form == "mask" else (None, pxq, pxt, C.byref(g))
        assert lib.svo_knn_match_gated(h, norm, pq, pt, dim, p(qo), p(to), 1, 2, *args, pi, pd, mem) == 0
        ctx.sync()
        m = mask if form == "mask" else mx.gate_mask(xq, xt, (2.0, 0.0, 12.5))
        wi, wd = mx.masked_from_keys(key, m, 2, norm)
        same((inner(ri, nq * 2, form).reshape(nq, 2), inner(rd, nq * 2, form).reshape(nq, 2)), (wi, wd), form)


def test_five_runs_two_contexts_and_the_old_calls_undisturbed(ctx):
    import torch

    rng = np.random.default_rng(21)
    norm, dim = mn.L2_F32, 6
    q, t = problem(rng, MQ + 1, 2049, dim, norm)
    key = mn.keys(q, t, norm)
    r = some_radius(key, norm, rng)
    xq, xt = lattice(rng, len(q)), lattice(rng, len(t))
    knn = mn.select(key, 2, norm)
    pairs = mn.ratio_pairs(*knn, xq, xt, 0.8)
    dq, dt = torch.from_numpy(q).cuda(), torch.from_numpy(t).cuda()

    def everything(c):
        out = [c.match_cross(q, t, norm=norm, mode=mx.MUTUAL), c.match_cross(dq, dt, norm=norm, mode=mx.CV)]
        same(c.knn_match(q, t, k=2, norm=norm), knn, "svo_knn_match between the new calls")
        out.append(c.radius_match(dq, dt, r, norm=norm)[1:])
        got = c.ratio_pairs(*c.knn_match(q, t, k=2, norm=norm), xq, xt, 0.8)
        assert all(np.array_equal(g, w) for g, w in zip(got, pairs)), "svo_ratio_pairs between the new calls"
        out.append(c.knn_match_gated(q, t, k=4, norm=norm, gate=(2.0, 0.0, 12.5), xy_query=xq, xy_train=xt))
        return [tuple(a.cpu().numpy() if hasattr(a, "cpu") else a for a in o) for o in out]

    first = everything(ctx)
    same(first[0], mx.cross_from_keys(key, norm, mx.MUTUAL))
    same(first[1], mx.cross_from_keys(key, norm, mx.CV))
    same(first[2], mx.radius_from_keys(key, norm, r)[1:])
    same(first[3], mx.masked_from_keys(key, mx.gate_mask(xq, xt, (2.0, 0.0, 12.5)), 4, norm))
    other = capi.Context(0)
    try:
        for c in (ctx, ctx, ctx, ctx, other):
            for a, b in zip(everything(c), first):
                same(a, b, "a repeated run")
    finally:
        other.close()


def test_smoke_program_equals_the_python_path(tmp_path, ctx, orc):
    """the adaptor's ORB branch with CROSS_CHECK_FLAG / EPIPOLAR_GATE_FLAG against the same calls from Python on the same pair"""
    import subprocess

    from ros_stereo_slam_amd import sequence, synth
    from test_match_ext_abi import build_smoke

    R, t = synth.corridor_trajectory(3, step=0.5)[0]
    left, right, _ = synth.Scene().stereo(R, t)
    exe = tmp_path / "match_ext_smoke"
    build_smoke(exe)
    files = [str(tmp_path / "left.ppm"), str(tmp_path / "right.ppm")]
    for f, im in zip(files, (left, right)):
        sequence.write_image(f, im)
    a, b = ctx.orb_extract_batch([left, right], n_features=1000)
    gate = (2.0, 0.0, 128.0)                               # epipolarRows, dx_min 0, maxDisparity: the adaptor's defaults
    band = mx.gate_mask(a[0], b[0], gate) != 0
    ci, _ = ctx.match_cross(a[4], b[4], norm=capi.MATCH_L2_U8, mode=capi.CROSS_CV)
    paired = np.flatnonzero(ci >= 0)
    want = {"cross": (a[0][paired], b[0][ci[paired]])}
    inside = paired[band[paired, ci[paired]]]
    want["both"] = (a[0][inside], b[0][ci[inside]])
    gi, gd = ctx.knn_match_gated(a[4], b[4], k=2, norm=capi.MATCH_L2_U8, gate=gate, xy_query=a[0], xy_train=b[0])
    want["gate"] = ctx.ratio_pairs(gi, gd, a[0], b[0], 0.8)[:2]
    pi, pd = ctx.knn_match(a[4], b[4], k=2, norm=capi.MATCH_L2_U8)
    want["plain"] = ctx.ratio_pairs(pi, pd, a[0], b[0], 0.8)[:2]
    P1, P2 = orc.stereo_projections(*synth.KITTI_K, synth.KITTI_BASELINE)
    for how, (p1, p2) in want.items():
        run = subprocess.run([str(exe), *files, how], check=True, capture_output=True, text=True, timeout=120)
        got = np.array([[float(v) for v in line.split()] for line in run.stdout.splitlines() if not line.startswith("#")],
                       np.float64).reshape(-1, 5).astype(np.float32)
        assert len(p1) >= 50, how
        assert np.array_equal(got[:, :2], p1), how
        assert np.array_equal(got[:, 2:5], orc.triangulate(P1, P2, p1, p2)[0], equal_nan=True), how
    dy = np.abs(want["gate"][0][:, 1] - want["gate"][1][:, 1])
    assert dy.max() <= 2.0 and len(want["both"][0]) <= len(want["cross"][0])
