"""svo_dedup_points and svo_replenish (csrc/replenish.hip) against the numpy restatement (tests/replenish_numpy.py), bit for bit:
every tile and workgroup seam, the last point of the last tile, the early-exit path, the boundaries, the x == 0 artefact, NaNs,
ref_idx; host and device memory behind guard bands; svo_replenish against the restatement and against the six-call composition it
replaces; every refusal; determinism; the neighbours on the same context; the prototype's loop on the library; the adaptors' smoke
program.  Every comparison is exact."""
import ctypes as C
import functools
import pathlib
import subprocess

import numpy as np
import pytest

import replenish_fixtures as rf
import replenish_numpy as rn
from ros_stereo_slam_amd import capi, prototype, synth

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parents[1]
BOX, DISC = rn.BOX, rn.DISC
MODES = [BOX, DISC]
GUARD = 0x5A


def want(c):
    return rn.dedup(c["ref"], c["new"], c["radius"], c["mode"], c["ref_idx"])


def got(ctx, c):
    return ctx.dedup_points(c["ref"], c["new"], c["radius"], c["mode"], c["ref_idx"])


def check(ctx, c, what):
    g, w = got(ctx, c), want(c)
    assert g.dtype == np.uint8 and g.shape == w.shape, what
    assert np.array_equal(g, w), (what, np.flatnonzero(g != w)[:8])
    assert np.array_equal(np.flatnonzero(g), np.flatnonzero(w))
    return g


@functools.lru_cache(maxsize=None)
def size_case(n_ref, n_new, mode):
    return rf.random_case(n_ref, n_new, mode, 100 + n_ref * 7 + n_new)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n_ref", rf.N_REF)
def test_every_size_equals_the_restatement(ctx, n_ref, mode):
    seen = set()
    for n_new in rf.N_NEW:
        seen |= set(check(ctx, size_case(n_ref, n_new, mode), (n_ref, n_new, mode)).tolist())     # wrapper: n_keep == keep.sum()
    assert seen == ({1} if n_ref == 0 else {0, 1})


@pytest.mark.parametrize("mode", MODES)
def test_last_point_of_the_last_tile(ctx, mode):
    keep = check(ctx, rf.last_of_last_tile(mode), "last of last")
    assert np.flatnonzero(keep == 0).tolist() == [200]


@pytest.mark.parametrize("mode", MODES)
def test_early_exit_path_terminates_and_is_right(ctx, mode):
    keep = check(ctx, rf.early_exit(mode), "early exit")
    assert not keep[:64].any() and np.flatnonzero(keep[64:] == 0).tolist() == [250 - 64]


def test_boundaries_artefact_nan_and_lists(ctx):
    assert check(ctx, rf.box_edge(), "box edge").tolist() == [1, 0, 1, 0, 1, 0, 1, 0, 1]
    assert check(ctx, rf.box_corner(BOX), "corner box").tolist() == [0, 0, 0]
    assert check(ctx, rf.box_corner(DISC), "corner disc").tolist() == [1, 0, 1]
    assert check(ctx, rf.disc_6_8(), "6 8").tolist() == [1, 0, 1, 1, 0, 1]
    for c, w in zip(rf.disc_sqrt_ulp(), ([1, 1, 1], [1, 1, 1], [0, 0, 1])):
        assert check(ctx, c, ("sqrt ulp", c["radius"])).tolist() == w
    assert check(ctx, rf.x_zero(BOX), "x zero box").tolist() == [0, 0, 1, 1, 1]
    assert check(ctx, rf.x_zero(DISC), "x zero disc").tolist() == [1, 1, 1, 1, 1]
    no_ref = dict(rf.x_zero(BOX), ref=np.zeros((0, 2), np.float32))
    assert check(ctx, no_ref, "x zero, no reference point").tolist() == [0, 0, 1, 1, 1]
    for mode in MODES:
        assert check(ctx, rf.nan_points(mode), "nan").tolist() == [1, 1, 1, 0, 1]
        for c in rf.listed(mode):
            check(ctx, c, ("listed", c["ref_idx"]))
        big = dict(size_case(2 * rf.T + 1, 257, mode))
        rng = np.random.default_rng(3)
        big["ref_idx"] = rng.integers(-50, 2 * rf.T + 60, 1500).tolist()          # repeats, disorder, both sides out of range, 2 tiles
        check(ctx, big, "long list")
    for r in (0.0, 1e-300, 1e300, float("inf")):
        for mode in MODES:
            check(ctx, dict(size_case(65, 64, mode), radius=r), ("radius", r))


@pytest.mark.parametrize("mode", MODES)
def test_device_memory_behind_guard_bands(ctx, mode):
    import torch

    for c in (size_case(2 * rf.T + 1, 257, mode), size_case(rf.T, 63, mode), rf.early_exit(mode), rf.listed(mode)[1], rf.listed(mode)[2]):
        n_new, pad = len(c["new"]), 64
        ref, new = torch.from_numpy(c["ref"]).cuda(), torch.from_numpy(c["new"]).cuda()
        idx = None if c["ref_idx"] is None else torch.tensor(c["ref_idx"] or [0], dtype=torch.int32).cuda()
        keep = torch.full((n_new + 2 * pad,), GUARD, dtype=torch.uint8).cuda()
        cnt = torch.full((3,), -7, dtype=torch.int32).cuda()
        torch.cuda.synchronize()
        capi._check(ctx.lib.svo_dedup_points(ctx._h, capi._ptr(ref), len(c["ref"]), capi._ptr(idx),
                                             0 if c["ref_idx"] is None else len(c["ref_idx"]), capi._ptr(new), n_new,
                                             C.c_double(c["radius"]), mode, C.c_void_p(keep.data_ptr() + pad),
                                             C.c_void_p(cnt.data_ptr() + 4), capi.MEM_DEVICE))
        ctx.sync()
        k, w = keep.cpu().numpy(), want(c)
        assert (k[:pad] == GUARD).all() and (k[pad + n_new:] == GUARD).all()
        assert np.array_equal(k[pad:pad + n_new], w)
        assert cnt.cpu().tolist() == [-7, int(w.sum()), -7]
        assert np.array_equal(ctx.dedup_points(ref, new, c["radius"], mode, c["ref_idx"]).cpu().numpy(), w)      # the wrapper's form


def test_host_memory_behind_guard_bands(ctx):
    c = size_case(rf.T + 1, 257, DISC)
    n_new, pad = 257, 32
    keep = np.full(n_new + 2 * pad, GUARD, np.uint8)
    cnt = (C.c_int * 3)(-7, -7, -7)
    capi._check(ctx.lib.svo_dedup_points(ctx._h, capi._ptr(c["ref"]), len(c["ref"]), None, 0, capi._ptr(c["new"]), n_new,
                                         C.c_double(5.0), DISC, C.c_void_p(keep.ctypes.data + pad), C.byref(cnt, 4), capi.MEM_HOST))
    assert (keep[:pad] == GUARD).all() and (keep[pad + n_new:] == GUARD).all() and np.array_equal(keep[pad:-pad], want(c))
    assert list(cnt) == [-7, int(want(c).sum()), -7]


# ---- svo_replenish ---------------------------------------------------------------------------------------------------------
def composition(ctx, c):
    """svo_dedup_points -> svo_compact -> svo_transform_points -> a host z > 0 mask -> svo_compact -> concatenation."""
    keep = ctx.dedup_points(c["ref"], c["new"], c["radius"], c["mode"])
    if len(keep) == 0:
        return c["ref"], c["ref_xyz"], 0, 0
    xy, xyz = ctx.compact(keep, c["new"], c["new_xyz"])
    moved = ctx.transform_points(c["Rt"], xyz).reshape(-1, 3)
    front = (moved[:, 2] > 0).astype(np.uint8)
    if len(front):
        xy, moved = ctx.compact(front, xy, moved)
    return (np.concatenate([c["ref"], xy.reshape(-1, 2)]), np.concatenate([c["ref_xyz"], moved.reshape(-1, 3)]),
            int((keep == 0).sum()), int((front == 0).sum()))


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


REPLENISH_SIZES = [(0, 0), (0, 65), (1, 1), (64, 0), (65, 63), (150, 257), (rf.T + 1, 1025), (2 * rf.T + 1, 256)]


@pytest.mark.parametrize("mode", MODES)
def test_replenish_equals_the_restatement_and_the_composition(ctx, mode):
    for n_ref, n_new in REPLENISH_SIZES:
        c = rf.replenish_case(n_ref, n_new, mode, 40 + n_ref + n_new)
        exp = rn.replenish(c["ref"], c["ref_xyz"], c["new"], c["new_xyz"], c["radius"], mode, c["Rt"])
        g = ctx.replenish(c["ref"], c["ref_xyz"], c["new"], c["new_xyz"], c["radius"], c["Rt"], mode)
        comp = composition(ctx, c)
        for other, name in ((exp, "restatement"), (comp, "composition")):
            assert same_bits(g[0], other[0]) and same_bits(g[1], other[1]), (n_ref, n_new, name)
            assert (g[2], g[3]) == (other[2], other[3]), (n_ref, n_new, name)
        assert g[2] + g[3] + (len(g[0]) - n_ref) == n_new
        assert same_bits(g[0][:n_ref], c["ref"]) and same_bits(g[1][:n_ref], c["ref_xyz"]) and (g[1][n_ref:, 2] > 0).all()
        if n_new >= 63:
            z = np.array([rn.move(c["Rt"], p)[2] for p in c["new_xyz"][want(dict(c, ref_idx=None)).astype(bool)]])
            assert (z == 0).any() and (z < 0).any() and (z > 0).any()          # the case holds what it is named for


@pytest.mark.parametrize("mem", ["host", "device"])
def test_replenish_leaves_the_other_rows_alone(ctx, mem):
    import torch

    n_ref, n_new, slack = 150, 257, 40
    c = rf.replenish_case(n_ref, n_new, BOX, 77)
    exp = rn.replenish(c["ref"], c["ref_xyz"], c["new"], c["new_xyz"], c["radius"], BOX, c["Rt"])
    cap = n_ref + n_new + slack
    xy, xyz = np.full((cap, 2), -3.5, np.float32), np.full((cap, 3), -4.5, np.float32)
    xy[:n_ref], xyz[:n_ref] = c["ref"], c["ref_xyz"]
    Rt = np.ascontiguousarray(c["Rt"], np.float64)
    if mem == "host":
        outs = (C.c_int * 5)(-7, -7, -7, -7, -7)
        capi._check(ctx.lib.svo_replenish(ctx._h, capi._ptr(xy), capi._ptr(xyz), n_ref, cap, capi._ptr(c["new"]), capi._ptr(c["new_xyz"]),
                                          n_new, C.c_double(5.0), BOX, capi._ptr(Rt), C.byref(outs, 4), C.byref(outs, 8),
                                          C.byref(outs, 12), capi.MEM_HOST))
        outs = list(outs)
    else:
        t_xy, t_xyz = torch.from_numpy(xy).cuda(), torch.from_numpy(xyz).cuda()
        t_outs = torch.full((5,), -7, dtype=torch.int32).cuda()
        ctx.replenish(t_xy, t_xyz, torch.from_numpy(c["new"]).cuda(), torch.from_numpy(c["new_xyz"]).cuda(), 5.0, Rt, BOX, n_ref=n_ref,
                      counts=t_outs[1:4])
        ctx.sync()
        xy, xyz, outs = t_xy.cpu().numpy(), t_xyz.cpu().numpy(), t_outs.cpu().tolist()
    n_out = len(exp[0])
    assert outs == [-7, n_out, exp[2], exp[3], -7]
    assert same_bits(xy[:n_out], exp[0]) and same_bits(xyz[:n_out], exp[1])
    assert (xy[n_out:] == -3.5).all() and (xyz[n_out:] == -4.5).all()
    # null outputs are legal
    xy2 = np.full((cap, 2), -3.5, np.float32)
    xyz2 = np.full((cap, 3), -4.5, np.float32)
    xy2[:n_ref], xyz2[:n_ref] = c["ref"], c["ref_xyz"]
    capi._check(ctx.lib.svo_replenish(ctx._h, capi._ptr(xy2), capi._ptr(xyz2), n_ref, cap, capi._ptr(c["new"]), capi._ptr(c["new_xyz"]),
                                      n_new, C.c_double(5.0), BOX, capi._ptr(Rt), None, None, None, capi.MEM_HOST))
    assert same_bits(xy2[:n_out], exp[0]) and (xy2[n_out:] == -3.5).all()


def test_capacity_refusal_leaves_the_arrays_untouched(ctx):
    n_ref, n_new = 65, 63
    c = rf.replenish_case(n_ref, n_new, DISC, 9)
    cap = n_ref + n_new - 1
    xy, xyz = np.full((cap + 8, 2), -3.5, np.float32), np.full((cap + 8, 3), -4.5, np.float32)
    xy[:n_ref], xyz[:n_ref] = c["ref"], c["ref_xyz"]
    before = (xy.copy(), xyz.copy())
    outs = (C.c_int * 3)(-7, -7, -7)
    Rt = np.ascontiguousarray(c["Rt"], np.float64)
    args = (capi._ptr(c["new"]), capi._ptr(c["new_xyz"]), n_new, C.c_double(5.0), DISC, capi._ptr(Rt), C.byref(outs, 0), C.byref(outs, 4),
            C.byref(outs, 8), capi.MEM_HOST)
    rc = ctx.lib.svo_replenish(ctx._h, capi._ptr(xy), capi._ptr(xyz), n_ref, cap, *args)
    assert rc == capi.SVO_ERR_CAPACITY and b"svo_replenish" in ctx.lib.svo_last_error()
    assert same_bits(xy, before[0]) and same_bits(xyz, before[1]) and list(outs) == [-7, -7, -7]
    assert ctx.lib.svo_replenish(ctx._h, capi._ptr(xy), capi._ptr(xyz), n_ref, cap + 1, *args) == capi.SVO_OK
    assert outs[0] == len(rn.replenish(c["ref"], c["ref_xyz"], c["new"], c["new_xyz"], 5.0, DISC, c["Rt"])[0])


def test_every_argument_refusal(ctx):
    lib, h = ctx.lib, ctx._h
    ref, new = np.full((4, 2), 7, np.float32), np.full((3, 2), 99, np.float32)
    keep, cnt = np.full(3, GUARD, np.uint8), (C.c_int * 1)(-9)
    idx = (C.c_int * 2)(0, 1)
    p = capi._ptr
    ok = dict(ctx=h, ref=p(ref), n_ref=4, idx=None, n_idx=0, new=p(new), n_new=3, r=5.0, mode=BOX, keep=p(keep), mem=capi.MEM_HOST)

    def dedup(**kw):
        a = dict(ok, **kw)
        return lib.svo_dedup_points(a["ctx"], a["ref"], a["n_ref"], a["idx"], a["n_idx"], a["new"], a["n_new"], C.c_double(a["r"]),
                                    a["mode"], a["keep"], cnt, a["mem"])

    bad = [dict(ctx=None), dict(n_ref=-1), dict(n_new=-1), dict(idx=idx, n_idx=-1), dict(r=-1.0), dict(r=-1e-300), dict(r=float("nan")),
           dict(mode=2), dict(mode=-1), dict(n_idx=2), dict(mem=2), dict(ref=None), dict(new=None), dict(keep=None),
           dict(n_ref=(1 << 28) + 1)]
    for kw in bad:
        assert dedup(**kw) == capi.SVO_ERR_ARG, kw
        assert b"svo_dedup_points" in lib.svo_last_error()
        assert (keep == GUARD).all() and cnt[0] == -9, kw
    assert dedup() == capi.SVO_OK and cnt[0] == 3 and keep.tolist() == [1, 1, 1]
    assert dedup(idx=idx, n_idx=0) == capi.SVO_OK and dedup(r=0.0) == capi.SVO_OK and dedup(r=float("inf")) == capi.SVO_OK
    assert keep.tolist() == [0, 0, 0]                      # an infinite radius: everything is a duplicate

    xy, xyz = np.full((8, 2), 7, np.float32), np.full((8, 3), 7, np.float32)
    new3, Rt = np.full((3, 3), 9, np.float32), np.ascontiguousarray(np.eye(3, 4))
    outs = (C.c_int * 3)(-9, -9, -9)
    ok = dict(ctx=h, xy=p(xy), xyz=p(xyz), n_ref=4, cap=8, new=p(new), new3=p(new3), n_new=3, r=5.0, mode=BOX, Rt=p(Rt), mem=capi.MEM_HOST)

    def repl(**kw):
        a = dict(ok, **kw)
        return lib.svo_replenish(a["ctx"], a["xy"], a["xyz"], a["n_ref"], a["cap"], a["new"], a["new3"], a["n_new"], C.c_double(a["r"]),
                                 a["mode"], a["Rt"], C.byref(outs, 0), C.byref(outs, 4), C.byref(outs, 8), a["mem"])

    bad = [dict(ctx=None), dict(n_ref=-1), dict(n_new=-1), dict(cap=-1), dict(r=-2.0), dict(r=float("nan")), dict(mode=7), dict(mem=-1),
           dict(Rt=None), dict(xy=None), dict(xyz=None), dict(new=None), dict(new3=None)]
    for kw in bad:
        assert repl(**kw) == capi.SVO_ERR_ARG, kw
        assert b"svo_replenish" in lib.svo_last_error()
        assert (xy == 7).all() and (xyz == 7).all() and list(outs) == [-9, -9, -9], kw
    assert repl(cap=6) == capi.SVO_ERR_CAPACITY and (xy == 7).all() and list(outs) == [-9, -9, -9]
    assert repl() == capi.SVO_OK and list(outs) == [7, 0, 0]


def test_five_identical_runs_two_contexts_and_the_neighbours(ctx):
    c = rf.replenish_case(2 * rf.T + 1, 257, DISC, 13)
    first = ctx.replenish(c["ref"], c["ref_xyz"], c["new"], c["new_xyz"], 5.0, c["Rt"], DISC)
    keep0 = got(ctx, dict(c, ref_idx=None))
    mask = (np.arange(300) % 3 != 0).astype(np.uint8)
    pts = np.random.default_rng(1).normal(0, 2, (300, 3)).astype(np.float32)
    compact0, moved0 = ctx.compact(mask, pts)[0].copy(), ctx.transform_points(c["Rt"], pts).copy()
    assert np.array_equal(compact0, pts[mask == 1])
    assert same_bits(moved0, np.array([rn.move(c["Rt"], q) for q in pts]))
    other = capi.Context(0)
    try:
        for k in range(5):
            who = other if k % 2 else ctx
            again = who.replenish(c["ref"], c["ref_xyz"], c["new"], c["new_xyz"], 5.0, c["Rt"], DISC)
            assert same_bits(again[0], first[0]) and same_bits(again[1], first[1]) and again[2:] == first[2:]
            assert np.array_equal(got(who, dict(c, ref_idx=None)), keep0)
            assert same_bits(ctx.compact(mask, pts)[0], compact0) and same_bits(ctx.transform_points(c["Rt"], pts), moved0)
    finally:
        other.close()


# ---- the prototype's loop ------------------------------------------------------------------------------------------------------
SIZE, K4, BASELINE, FRAMES = (640, 240), (360.0, 360.0, 320.0, 120.0), 0.54, 7


@functools.lru_cache(maxsize=None)
def stereo_frames():
    poses = synth.corridor_trajectory(FRAMES, step=0.5)
    lefts, rights = synth.stereo_torch(synth.Scene(), poses, K=K4, size=SIZE, channels=1, baseline=BASELINE)
    return [(l.cpu().numpy().reshape(SIZE[1], SIZE[0]), r.cpu().numpy().reshape(SIZE[1], SIZE[0])) for l, r in zip(lefts, rights)]


def inside_box(q, ref, r):
    d = np.abs(ref.astype(np.float64)[None, :, :] - q.astype(np.float64)[:, None, :])
    return ((d[..., 0] < r) & (d[..., 1] < r)).any(axis=1)


def test_vis_odometry_steps_are_the_capi_calls(ctx):
    frames = stereo_frames()
    vo = prototype.VisOdometry(ctx, K4, BASELINE, seed=3)
    bare = prototype.VisOdometry(ctx, K4, BASELINE, seed=3, replenish=False)
    n0 = vo.initializeSequence(*frames[0])
    assert n0 == bare.initializeSequence(*frames[0]) and n0 > 50
    prev_img = frames[0][0]
    for k in range(1, FRAMES):                                   # six steps
        left, right = frames[k]
        ref2d, ref3d = vo.referencePoints2D.copy(), vo.referencePoints3D.copy()
        assert vo.referenceImage is prev_img
        R, t, n_out, n_dup, n_behind = vo.step(left, right)
        # the same calls, made here from the state before the step
        p3, _, trk = vo.trackPointsFrame2Frame(prev_img, left, ref2d, ref3d)
        cnt, rvec, tvec, inl, _ = ctx.pnp_ransac(p3, trk, K4, 100, 8.0, 0.99, 3)
        Rm = prototype.rodrigues(rvec)
        assert np.array_equal(R, Rm.T) and np.array_equal(t, -Rm.T @ tvec)
        held2d, held3d = trk[inl], p3[inl]
        new3d, new2d = vo.sparseStereoTriangulate(left, right)
        e2d, e3d, e_dup, e_behind = ctx.replenish(held2d, held3d, new2d, new3d, 5, np.hstack((Rm.T, (-Rm.T @ tvec).reshape(3, 1))), BOX)
        assert same_bits(vo.referencePoints2D, e2d) and same_bits(vo.referencePoints3D, e3d)
        assert (n_out, n_dup, n_behind) == (len(e2d), e_dup, e_behind) and n_dup + n_behind + (n_out - cnt) == len(new2d)
        # the inlier set leads, nothing appended duplicates it, everything appended lies in front
        assert same_bits(vo.referencePoints2D[:cnt], held2d) and same_bits(vo.referencePoints3D[:cnt], held3d)
        added2d, added3d = vo.referencePoints2D[cnt:], vo.referencePoints3D[cnt:]
        assert len(added2d) > 0 and not inside_box(added2d, held2d, 5.0).any() and (added3d[:, 2] > 0).all()
        # and it is what the prototype's own order of the steps gives: filter inside the triangulation, then move and append
        f3d, f2d = vo.sparseStereoTriangulate(left, right, refPts=held2d)
        assert same_bits(f2d, new2d[vo.removeDuplicate(new2d, held2d)])
        moved = ctx.transform_points(np.hstack((Rm.T, (-Rm.T @ tvec).reshape(3, 1))), f3d).reshape(-1, 3)
        assert same_bits(added2d, f2d[moved[:, 2] > 0]) and same_bits(added3d, moved[moved[:, 2] > 0])
        bare.step(left, right)
        prev_img = left
    assert len(vo.referencePoints2D) > len(bare.referencePoints2D), "the top-up happens"
    assert len(vo.path) == FRAMES - 1
    again = prototype.VisOdometry(ctx, K4, BASELINE, seed=3).trackSequence(frames)
    assert len(again) == FRAMES - 1 and np.array_equal(again[-1][1], vo.path[-1][1]) and again[-1][2] == len(vo.referencePoints2D)


def test_adaptor_smoke_program(tmp_path):
    exe = tmp_path / "replenish_smoke"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(ROOT / "tests" / "cpp" / "replenish_smoke.cpp"),
                    f"-L{ROOT / 'ros_stereo_slam_amd'}", "-l:libsvo_hip.so", f"-Wl,-rpath,{ROOT / 'ros_stereo_slam_amd'}", "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "replenish smoke ok" in out.stdout, (out.returncode, out.stdout, out.stderr)
    assert "# all 1 3\n" in out.stdout and "# odd 1 3 4\n" in out.stdout and "# none 0 1 2 3 4 5\n" in out.stdout
