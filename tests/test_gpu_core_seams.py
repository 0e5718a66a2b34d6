"""The kernels that run on every frame -- svo_compact, svo_anms, svo_get_colors, svo_transform_points, svo_triangulate, svo_fransac,
svo_pnp_ransac, svo_ba_3d2d, svo_sor_filter -- at every tile, wave and workgroup seam of tests/core_fixtures.py: against the oracle
bit for bit and against the plain numpy definitions of tests/core_numpy.py, in host and in device memory, behind sentinel-filled
guard bands, at mask pointers of every alignment, over repeated runs and on two contexts.  tests/test_core_numpy.py shows on the CPU
that these inputs are not vacuous."""
import ctypes as C

import numpy as np
import pytest

import core_fixtures as cf
import core_numpy as cn
from ba_fixtures import problem as ba_problem
from geom_fixtures import BASELINE, K4
from ros_stereo_slam_amd import capi
from test_oracle_sor import cloud

pytestmark = pytest.mark.gpu

GUARD = 64                                   # elements of sentinel on either side of every device output
FILL = {"float32": -12345.5, "int32": -77, "uint8": 0xA5}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def dev(a):
    import torch

    return torch.from_numpy(np.array(a, order="C")).cuda()       # a copy: the shared inputs are read-only


class Banded:
    """n elements of device memory between two guard bands, all filled with a sentinel."""

    def __init__(self, n, dtype="float32"):
        import torch

        self.n, self.fill = n, FILL[dtype]
        self.buf = torch.full((GUARD + n + GUARD,), self.fill, dtype=getattr(torch, dtype), device="cuda")
        self.ptr = C.c_void_p(self.buf.data_ptr() + GUARD * self.buf.element_size())

    def read(self, written, what):
        """The first ``written`` elements; the rest and both guard bands must still hold the sentinel."""
        host = self.buf.cpu().numpy()
        assert (host[:GUARD] == self.fill).all() and (host[GUARD + self.n:] == self.fill).all(), (what, "a guard band was written")
        assert (host[GUARD + written:GUARD + self.n] == self.fill).all(), (what, "rows past the count were written")
        return host[GUARD:GUARD + written].copy()


def _launch(ctx, call):
    """A device-form call: the inputs are complete (torch's stream), the call is queued, the context's stream drains."""
    import torch

    torch.cuda.synchronize()
    assert call() == capi.SVO_OK, ctx.lib.svo_last_error()
    ctx.sync()


def _vp(t):
    return C.c_void_p(t.data_ptr())


# ------------------------------------------------------------------------------------------------------------------ svo_compact
def _compact_device(ctx, mask, arrays, offset):
    """Device form: the mask ``offset`` bytes behind a 16-byte boundary, banded outputs, the count in a device int."""
    import torch

    n = len(mask)
    mbuf = torch.full((n + 48,), 0xA5, dtype=torch.uint8, device="cuda")
    start = (-mbuf.data_ptr()) % 16 + offset
    mview = mbuf[start:start + n]
    assert (mbuf.data_ptr() + start) % 16 == offset
    if n:
        mview.copy_(torch.from_numpy(mask))
    ins = [dev(a) for a in arrays]
    outs = [Banded(a.size) for a in arrays]
    cnt = Banded(1, "int32")
    args = []
    for k in range(3):
        args += [_vp(ins[k]), arrays[k].shape[1], outs[k].ptr] if k < len(arrays) else [None, 0, None]
    _launch(ctx, lambda: ctx.lib.svo_compact(ctx._h, C.c_void_p(mbuf.data_ptr() + start), n, *args, cnt.ptr, capi.MEM_DEVICE))
    k = int(cnt.read(1, "count")[0])
    assert 0 <= k <= n, k
    return [o.read(k * a.shape[1], ("compact", n, offset)).reshape(k, a.shape[1]) for o, a in zip(outs, arrays)]


@pytest.mark.parametrize("n", cf.sizes("compact"))
def test_compact_every_seam_mask_and_alignment(ctx, n):
    arrays = cf.compact_arrays(n)                          # strides 2 / 3 / 2
    for kind in cf.MASK_KINDS:
        mask = cf.compact_mask(n, kind)
        ref = cn.compact(mask, *arrays)
        got = ctx.compact(mask, *arrays)
        assert all(same_bits(g, r) for g, r in zip(got, ref)), (n, kind, "host", len(got[0]), len(ref[0]))
        (only,) = ctx.compact(mask, arrays[1])
        assert same_bits(only, ref[1]), (n, kind, "host, one array")
        for offset in (0, 1, 4, 15):                        # 0: the 16-byte prefix count; the others: byte by byte
            got = _compact_device(ctx, mask, arrays, offset)
            assert all(same_bits(g, r) for g, r in zip(got, ref)), (n, kind, "device", offset, len(got[0]), len(ref[0]))
        (only,) = _compact_device(ctx, mask, arrays[:1], 4)
        assert same_bits(only, ref[0]), (n, kind, "device, one array")


# ------------------------------------------------------------------------------------------------------------------ svo_anms
def _anms_device(ctx, xy, resp, keep):
    n = len(resp)
    dxy, dresp = dev(xy), dev(resp)
    idx, cnt = Banded(n, "int32"), Banded(1, "int32")
    _launch(ctx, lambda: ctx.lib.svo_anms(ctx._h, _vp(dxy), _vp(dresp), n, keep, idx.ptr, cnt.ptr, capi.MEM_DEVICE))
    k = int(cnt.read(1, "count")[0])
    assert 0 <= k <= n, k
    return idx.read(k, ("anms", n, keep))


@pytest.mark.parametrize("n", cf.sizes("anms"))
def test_anms_every_seam_keep_and_input(ctx, orc, n):
    for kind in cf.ANMS_KINDS:
        xy, resp = cf.anms_input(kind, n)
        order, r2 = cn.anms_radii(xy, resp)
        for keep in cf.anms_keeps(n):
            ref, _ = orc.anms(xy, resp, keep)
            assert np.array_equal(ref, cn.anms_select(order, r2, keep)), (kind, n, keep, "oracle against numpy")
            got = ctx.anms(xy, resp, keep)
            assert same_bits(got, ref), (kind, n, keep, "host", len(got), len(ref))
            got = _anms_device(ctx, xy, resp, keep)
            assert same_bits(got, ref), (kind, n, keep, "device", len(got), len(ref))


def test_anms_of_nothing_writes_a_zero_count(ctx):
    """As svo_compact at n = 0: the device count is an output of an empty call too, not what the last call left there."""
    idx, cnt = Banded(4, "int32"), Banded(1, "int32")
    _launch(ctx, lambda: ctx.lib.svo_anms(ctx._h, None, None, 0, 5, idx.ptr, cnt.ptr, capi.MEM_DEVICE))
    assert int(cnt.read(1, "count")[0]) == 0 and len(idx.read(0, "anms of nothing")) == 0
    assert len(ctx.anms(np.zeros((0, 2), np.float32), np.zeros(0, np.float32), 5)) == 0


@pytest.mark.parametrize("n", cf.sizes("anms"))
def test_anms_five_identical_runs(ctx, n):
    for kind in ("lattice", "mixed_sign"):
        xy, resp = cf.anms_input(kind, n)
        runs = [ctx.anms(xy, resp, n // 2).tobytes() + _anms_device(ctx, xy, resp, n // 2).tobytes() for _ in range(5)]
        assert all(r == runs[0] for r in runs[1:]) and len(runs[0]) >= 8, (kind, n)


# ------------------------------------------------------------------------------------------------------------------ svo_get_colors
def _colors_device(ctx, pyr, xy):
    dxy = dev(xy)
    out = Banded(3 * len(xy))
    _launch(ctx, lambda: ctx.lib.svo_get_colors(ctx._h, pyr._h, _vp(dxy), len(xy), out.ptr, capi.MEM_DEVICE))
    return out.read(3 * len(xy), ("colors", len(xy))).reshape(-1, 3)


@pytest.mark.parametrize("w,h,c", cf.COLOR_IMAGES)
def test_get_colors_clamp_truncation_and_pitch(ctx, orc, w, h, c):
    img = cf.color_image(w, h, c)
    pyr = ctx.pyramid(w, h, c).build(np.ascontiguousarray(img))
    try:
        edge = cf.color_edge_points(w, h)
        sets = [cf.color_points(w, h, n) for n in cf.sizes("colors")[1:]] + [edge] + [p[None] for p in edge]   # n = 1: each edge point
        for xy in sets:
            ref = orc.get_colors(img, xy)
            assert np.array_equal(ref, cn.get_colors(img, xy)), (w, h, c, len(xy), "oracle against numpy")
            got = ctx.get_colors(pyr, xy)
            assert same_bits(got, ref), (w, h, c, len(xy), "host", xy[(got != ref).any(axis=1)])
            got = _colors_device(ctx, pyr, xy)
            assert same_bits(got, ref), (w, h, c, len(xy), "device", xy[(got != ref).any(axis=1)])
    finally:
        pyr.close()


# ------------------------------------------------------------------------------------------------------------------ svo_transform_points
@pytest.mark.parametrize("n", cf.sizes("points"))
def test_transform_points_every_seam(ctx, orc, n):
    pts = cf.transform_input(n)
    ref = orc.transform_points(cf.RT, pts)
    got = ctx.transform_points(cf.RT, pts)
    assert same_bits(got, ref), (n, "host")
    dpts, out = dev(pts), Banded(3 * n)
    Rt = np.ascontiguousarray(cf.RT, np.float64)
    _launch(ctx, lambda: ctx.lib.svo_transform_points(ctx._h, C.c_void_p(Rt.ctypes.data), _vp(dpts), n, out.ptr, capi.MEM_DEVICE))
    assert same_bits(out.read(3 * n, ("transform", n)).reshape(n, 3), ref), (n, "device")
    d = cf.ulp_distance(got, cn.transform_points(cf.RT, pts))
    assert n == 0 or d.max() <= 1, f"n = {n}: {int((d > 0).sum())} of {d.size} components differ from float64 numpy, the worst by {int(d.max())} ulp"


# ------------------------------------------------------------------------------------------------------------------ svo_triangulate
@pytest.mark.parametrize("n", cf.sizes("points"))
def test_triangulate_every_seam_with_degenerate_pairs_at_the_wave_ends(ctx, orc, n):
    P1, P2 = capi.stereo_projections(*K4, BASELINE)
    a, b, zero, neg = cf.tri_input(n)
    oxyz, oh = orc.triangulate(P1, P2, a, b)
    gxyz, gh = ctx.triangulate(P1, P2, a, b)
    assert same_bits(gh, oh) and same_bits(gxyz, oxyz), (n, "host", np.flatnonzero((gh != oh).any(axis=1)))
    ref_xyz, ref_v = cn.triangulate(P1, P2, a, b)
    cf.check_dlt(gxyz, gh, ref_xyz, ref_v, zero, ("gpu", n))
    if n:
        assert gxyz.shape == (n, 3) and (gxyz[neg, 2] < 0).all()
    p1, p2 = np.ascontiguousarray(P1), np.ascontiguousarray(P2)
    pp = (C.c_void_p(p1.ctypes.data), C.c_void_p(p2.ctypes.data))
    # host form without the homogeneous output
    xyz = np.full((max(n, 1), 3), FILL["float32"], np.float32)
    assert ctx.lib.svo_triangulate(ctx._h, *pp, C.c_void_p(a.ctypes.data), C.c_void_p(b.ctypes.data), n, C.c_void_p(xyz.ctypes.data),
                                   None, capi.MEM_HOST) == capi.SVO_OK
    assert same_bits(xyz[:n], oxyz) and (xyz[n:] == FILL["float32"]).all(), (n, "host, no homogeneous output")
    # device form, the homogeneous output requested and left out
    da, db = dev(a), dev(b)
    for want_h in (True, False):
        dxyz, dh = Banded(3 * n), Banded(4 * n)
        _launch(ctx, lambda: ctx.lib.svo_triangulate(ctx._h, *pp, _vp(da), _vp(db), n, dxyz.ptr, dh.ptr if want_h else None,
                                                     capi.MEM_DEVICE))
        assert same_bits(dxyz.read(3 * n, ("triangulate", n)).reshape(n, 3), oxyz), (n, "device", want_h)
        assert same_bits(dh.read(4 * n if want_h else 0, ("triangulate h", n)).reshape(-1, 4), oh if want_h else oh[:0]), (n, want_h)


# ------------------------------------------------------------------------------------------------------------------ svo_fransac
@pytest.mark.parametrize("thr", cf.FRANSAC_THRESHOLDS)
@pytest.mark.parametrize("n", cf.sizes("fransac"))
def test_fransac_between_the_small_sample_branch_and_800_pairs(ctx, orc, n, thr):
    x1, x2, gt, seed = cf.fransac_case(n, thr)
    gc, gmask, gF, git = ctx.fransac(x1, x2, thr, seed=seed)
    oc, omask, oF, oit = orc.fransac(x1, x2, thr, seed=seed)
    assert (git, gc) == (oit, oc), (n, thr, git, oit, gc, oc)
    assert same_bits(gmask, omask) and same_bits(gF, oF), (n, thr, int((gmask != omask).sum()))
    assert 0 < gc < n


# ------------------------------------------------------------------------------------------------------------------ svo_pnp_ransac
@pytest.mark.parametrize("n", cf.sizes("pnp"))
def test_pnp_ransac_between_the_minimal_sample_and_800_points(ctx, orc, n):
    X, x, gt, err, seed = cf.pnp_case(n)
    gc, grv, gtv, ginl, git = ctx.pnp_ransac(X, x, K4, reproj_err=err, seed=seed)
    oc, orv, otv, oinl, oit = orc.pnp_ransac(X, x, K4, reproj_err=err, seed=seed)
    assert (git, gc) == (oit, oc), (n, git, oit, gc, oc)
    assert same_bits(ginl, oinl) and same_bits(grv, orv) and same_bits(gtv, otv), (n, grv - orv, gtv - otv)
    assert gc >= 5
    cnt, *_ = ctx.pnp_ransac(X[:4], x[:4], K4, reproj_err=err, seed=seed)      # fewer than a sample: still refused
    assert cnt == 0


# ------------------------------------------------------------------------------------------------------------------ svo_ba_3d2d
@pytest.mark.parametrize("n", cf.sizes("ba"))
def test_ba_where_the_fixed_order_reduction_changes_shape(ctx, orc, n):
    """The assertions of tests/test_gpu_ba.py::test_ba_matches_oracle at the seams of the BA_T-thread workgroup."""
    uv, X, R0, t0, (Rw, tw) = ba_problem(n, seed=n)
    for its in (0, 1, 6):
        tg, Rg, Xg, ig = ctx.ba_3d2d(uv, X, K4, R0, t0, iterations=its)
        to, Ro, Xo, io = orc.ba_3d2d(uv, X, K4, R0, t0, iterations=its)
        assert ig["iterations"] == io["iterations"] and ig["trials"] == io["trials"], (n, its, ig, io)
        assert ig["chi2_before"] == pytest.approx(io["chi2_before"], rel=1e-13)
        assert ig["lambda_final"] == pytest.approx(io["lambda_final"], rel=1e-9)
        assert np.abs(tg - to).max() < 1e-9 and np.abs(Rg - Ro).max() < 1e-10
        assert np.abs(Xg - Xo).max() < 1e-7
    tg, Rg, Xg, ig = ctx.ba_3d2d(uv, X, K4, R0, t0)
    to, Ro, Xo, io = orc.ba_3d2d(uv, X, K4, R0, t0)
    assert np.abs(tg - to).max() < 1e-8 and np.abs(Rg - Ro).max() < 1e-9


# ------------------------------------------------------------------------------------------------------------------ svo_sor_filter
@pytest.mark.parametrize("n,k", cf.SOR_CASES)
def test_sor_neighbour_count_below_at_and_above_the_cloud(ctx, orc, n, k):
    """The assertions of tests/test_gpu_sor.py::test_matches_oracle."""
    xyz, col = cloud(n, seed=n + 1, outliers=n // 40)
    xo, co, mo = orc.sor_filter(xyz, col, mean_k=k, stddev_mul=0.01, z_limit=500.0)
    xg, cg, mg = ctx.sor_filter(xyz, col, mean_k=k, stddev_mul=0.01, z_limit=500.0)
    assert len(mg) == len(mo)
    assert np.array_equal(mg, mo)
    assert np.array_equal(xg, xo) and np.array_equal(cg, co)
    assert 0 < len(xg) <= n


# ------------------------------------------------------------------------------------------------------------------ neighbours
def test_two_contexts_alternating_compaction_and_anms(ctx):
    """The scratch buffers are per context: two contexts that take turns at different sizes give what each gives alone."""
    jobs = {}
    for n in (129, 1025, 257, 513):
        jobs["compact", n] = (cf.compact_mask(n, "odd"), cf.compact_arrays(n))
        jobs["anms", n] = cf.anms_input("lattice", n) + (n // 2,)

    def run(c, op, n):
        if op == "compact":
            mask, arrays = jobs[op, n]
            return b"".join(o.tobytes() for o in c.compact(mask, *arrays))
        return c.anms(*jobs[op, n]).tobytes()

    alone = {key: run(ctx, *key) for key in jobs}
    assert all(len(v) > 100 for v in alone.values())
    other = capi.Context(0)
    try:
        for _ in range(2):
            for a, b in ((("compact", 1025), ("anms", 513)), (("anms", 257), ("compact", 129)), (("anms", 1025), ("anms", 129)),
                         (("compact", 257), ("compact", 513))):
                assert run(ctx, *a) == alone[a] and run(other, *b) == alone[b], (a, b)
                assert run(other, *a) == alone[a] and run(ctx, *b) == alone[b], (b, a)
    finally:
        other.close()
