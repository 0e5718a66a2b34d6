"""Grey frames stored as BGR: the pyramid build leaves a "channels agree" word on the device (pyramid.hip), and the tracker
sums one channel of such a pair and multiplies its exact integer totals by 3 before their one rounding (lk.hip).  Nothing
may change: every result here is compared bit for bit with the oracle's THREE-channel LK, and with the same launch under
SVO_LK_MONO=0.  The switches are read once per process, so every other setting runs in a fresh child process (this file,
run as a script).  The gated build and the 16-job launch go through svo_pyramid_build_gated / svo_lk_track_jobs.

Shapes: 96 x 64 x 3 with 4 levels, the smallest the pyramid accepts with room for a 21-pixel window on level 3."""
import os
import pathlib
import subprocess
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

pytestmark = pytest.mark.gpu

W, H = 96, 64


def _pair(colour=False, seed=5, shift=(1.3, -0.7)):
    from ros_stereo_slam_amd import synth

    if colour:
        return synth.textured_pair(W, H, 3, shift=shift, seed=seed, colour=True)
    a, b = synth.textured_pair(W, H, 1, shift=shift, seed=seed)
    a, b = a.reshape(H, W, 1), b.reshape(H, W, 1)
    return np.ascontiguousarray(np.repeat(a, 3, 2)), np.ascontiguousarray(np.repeat(b, 3, 2))


def _points():
    """About 200: the lattice (integer positions, identity path at the levels whose scale divides them), fractional points,
    points within a window of every border and points outside the image."""
    rng = np.random.default_rng(23)
    gx, gy = np.meshgrid(np.arange(8, W - 7, 8, dtype=np.float32), np.arange(8, H - 7, 8, dtype=np.float32))
    lat = np.stack([gx.ravel(), gy.ravel()], 1)
    frac = rng.uniform([12, 12], [W - 12, H - 12], (90, 2)).astype(np.float32)
    edge = rng.uniform([-6, -6], [W + 6, H + 6], (40, 2)).astype(np.float32)
    return np.concatenate([lat, frac, edge])


def _bits(o, st, err, me):
    return (np.ascontiguousarray(o, np.float32).view(np.uint32), np.asarray(st, np.uint8),
            np.ascontiguousarray(err, np.float32).view(np.uint32), np.ascontiguousarray(me, np.float32).view(np.uint32))


def _same(got, want, what):
    for g, w_, name in zip(got, want, ("next_pts", "status", "err", "min_eig")):
        assert np.array_equal(g, w_), f"{what}: {name} differs"


def _track(ctx, a, b, pts):
    pa, pb = ctx.pyramid(W, H, a.shape[2]).build(a), ctx.pyramid(W, H, b.shape[2]).build(b)
    words = (pa.is_mono(), pb.is_mono())
    res = _bits(*ctx.lk_track(pa, pb, pts))
    pa.close()
    pb.close()
    return words, res


@pytest.fixture(scope="module")
def ctx():
    import torch

    torch.cuda.is_available()
    from ros_stereo_slam_amd import capi

    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def grey(orc):
    a, b = _pair()
    pts = _points()
    want = _bits(*orc.lk_track(a, b, pts))
    assert want[1].mean() >= 0.6, "the oracle itself should track most of the points of the grey pair"
    return a, b, pts, want


def _child(out):
    import torch

    torch.cuda.is_available()
    from ros_stereo_slam_amd import capi

    ctx = capi.Context(0)
    a, b = _pair()
    pts = _points()
    words, res = _track(ctx, a, b, pts)
    # the same launch without the err output: the kernel variant without the level-0 residual
    pa, pb = ctx.pyramid(W, H, 3).build(a), ctx.pyramid(W, H, 3).build(b)
    n = len(pts)
    dp = torch.from_numpy(pts).cuda()
    do, ds, dm = torch.zeros(n, 2, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda"), torch.zeros(n, device="cuda")
    ctx.lk_track_device(pa, pb, dp, n, do, ds, None, dm)
    ctx.sync()
    np.savez(out, words=np.array(words), o=res[0], st=res[1], err=res[2], me=res[3], o2=do.cpu().numpy().view(np.uint32),
             st2=ds.cpu().numpy(), me2=dm.cpu().numpy().view(np.uint32))
    pa.close()
    pb.close()
    ctx.close()


@pytest.mark.parametrize("env", [{}, {"SVO_LK_MONO": "0"}, {"SVO_LK_LATTICE": "0"}, {"SVO_LK_CELL_CACHE": "0"}],
                         ids=["default", "mono0", "lattice0", "cellcache0"])
def test_grey_pair_equals_the_three_channel_oracle_under_every_switch(grey, env, tmp_path):
    a, b, pts, want = grey
    out = tmp_path / "r.npz"
    r = subprocess.run([sys.executable, __file__, str(out)], env=dict(os.environ, **env), capture_output=True, text=True,
                       timeout=300, cwd=str(ROOT))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    d = np.load(out)
    assert d["words"].tolist() == [True, True]  # the word does not depend on the tracker's switch
    _same((d["o"], d["st"], d["err"], d["me"]), want, f"{env}")
    # without err: the other kernel variant
    assert np.array_equal(d["o2"].reshape(-1, 2), want[0]) and np.array_equal(d["st2"], want[1]) and np.array_equal(d["me2"], want[3])


def test_grey_and_colour_pairs_report_their_words_and_take_the_full_path(ctx, orc, grey):
    ga, gb, pts, _ = grey
    ca, cb = _pair(colour=True)
    for a, b, words in ((ga, cb, (True, False)), (ca, gb, (False, True)), (ca, cb, (False, False))):
        got_words, got = _track(ctx, a, b, pts)
        assert got_words == words
        _same(got, _bits(*orc.lk_track(a, b, pts)), f"words {words}")


# one channel byte changed by 1: the first pixel, the last pixel of the last row, a pixel whose three bytes straddle a
# dword boundary (pixel 1 of a row: bytes 3, 4, 5 -- whatever the row's alignment, one of pixels 1, 2 straddles), the last
# pixel of row 0, and an interior pixel of the last row (its final bytes are copied byte by byte)
@pytest.mark.parametrize("y,x,ch", [(0, 0, 0), (0, 0, 2), (H - 1, W - 1, 2), (H - 1, W - 1, 0), (5, 1, 1), (5, 2, 2), (0, W - 1, 1),
                                    (H - 1, W - 2, 0), (H - 1, 0, 1), (1, 0, 0)])
def test_one_byte_off_grey_is_colour(ctx, orc, grey, y, x, ch):
    ga, gb, pts, _ = grey
    a = ga.copy()
    a[y, x, ch] = a[y, x, ch] + 1 if a[y, x, ch] < 255 else 254
    words, got = _track(ctx, a, gb, pts)
    assert words == (False, True)
    _same(got, _bits(*orc.lk_track(a, gb, pts)), f"byte ({y}, {x}, {ch})")
    words, got = _track(ctx, ga, a, pts)
    assert words == (True, False)
    _same(got, _bits(*orc.lk_track(ga, a, pts)), f"byte ({y}, {x}, {ch}) in the second image")


def test_the_word_follows_the_builds_of_one_pyramid(ctx, grey):
    ga, gb, _, _ = grey
    ca, _ = _pair(colour=True)
    p = ctx.pyramid(W, H, 3)
    assert not p.is_mono()  # never built
    for img, want in ((ga, True), (ca, False), (gb, True), (ca, False), (ga, True), (gb, True)):
        assert p.build(img).is_mono() == want
    p.close()


def test_a_gated_build_leaves_the_word_and_the_levels_alone(ctx, grey):
    import torch

    ga, gb, _, _ = grey
    ca, _ = _pair(colour=True)
    shut, open_ = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.ones(1, dtype=torch.int32, device="cuda")
    dev = {k: torch.from_numpy(v).cuda() for k, v in (("ga", ga), ("gb", gb), ("ca", ca))}
    p = ctx.pyramid(W, H, 3)
    seq = (("ga", open_, True, ga), ("ca", open_, False, ca), ("gb", open_, True, gb), ("ca", shut, True, gb),
           ("ga", open_, True, ga), ("ca", open_, False, ca), ("ga", shut, False, ca), ("gb", None, True, gb))
    for name, gate, want, holds in seq:
        assert p.build_gated(dev[name], gate).is_mono() == want, (name, gate)
        assert np.array_equal(p.level(0), holds)
    p.close()


def test_sixteen_jobs_of_one_launch_equal_their_own_launches(ctx, grey):
    """Mono and colour jobs side by side (the choice is per job) and a gated job, which writes nothing."""
    import torch

    ga, gb, pts, _ = grey
    ca, cb = _pair(colour=True)
    ga2, gb2 = _pair(seed=8, shift=(-0.8, 1.1))
    pairs = [(ga, gb), (ca, cb), (ga, cb), (ca, gb), (ga2, gb2), (gb, ga), (cb, ca), (gb2, ga2)] * 2
    n = len(pts)
    dp = torch.from_numpy(pts).cuda()
    pyrs = [(ctx.pyramid(W, H, 3).build(a), ctx.pyramid(W, H, 3).build(b)) for a, b in pairs]
    assert [(pa.is_mono(), pb.is_mono()) for pa, pb in pyrs[:8]] == [(True, True), (False, False), (True, False), (False, True),
                                                                   (True, True), (True, True), (False, False), (True, True)]
    GATED = 5

    def outputs():
        return (torch.full((n, 2), -7.0, device="cuda"), torch.full((n,), 9, dtype=torch.uint8, device="cuda"),
                torch.full((n,), -7.0, device="cuda"), torch.full((n,), -7.0, device="cuda"))

    for with_err in (True, False):
        outs = [outputs() for _ in pairs]
        gates = [torch.tensor([0 if k == GATED else 1], dtype=torch.int32, device="cuda") for k in range(16)]
        ctx.lk_track_jobs([(pa, pb, dp, o[0], o[1], o[2] if with_err else None, o[3], g if k % 3 != 1 else None)
                           for k, ((pa, pb), o, g) in enumerate(zip(pyrs, outs, gates))])
        ctx.sync()
        for k, ((pa, pb), o) in enumerate(zip(pyrs, outs)):
            got = [t.cpu().numpy() for t in o]
            if k == GATED:
                assert (got[0] == -7).all() and (got[1] == 9).all() and (got[2] == -7).all() and (got[3] == -7).all()
                continue
            want = _bits(*ctx.lk_track(pa, pb, pts))
            assert np.array_equal(got[0].view(np.uint32), want[0]) and np.array_equal(got[1], want[1]), f"job {k}"
            assert np.array_equal(got[3].view(np.uint32), want[3]), f"job {k}"
            if with_err:
                assert np.array_equal(got[2].view(np.uint32), want[2]), f"job {k}"
    for pa, pb in pyrs:
        pa.close()
        pb.close()


def test_a_one_channel_pyramid_never_reports_mono(ctx, orc, grey):
    ga, gb, pts, _ = grey
    a1, b1 = np.ascontiguousarray(ga[..., :1]), np.ascontiguousarray(gb[..., :1])
    words, got = _track(ctx, a1, b1, pts)
    assert words == (False, False)
    _same(got, _bits(*orc.lk_track(a1, b1, pts)), "C == 1")


if __name__ == "__main__":
    _child(sys.argv[1])
