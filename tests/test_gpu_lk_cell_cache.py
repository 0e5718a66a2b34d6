"""The tracker's cell cache (lk.hip, step 2: the iteration loop keeps a lane's column pairs for as long as the guess stays in
its pixel cell of the staged tile) must not change a single bit.  SVO_LK_CELL_CACHE=0 reloads and pairs the two tile rows in
every iteration; the switch is read once per process, so each setting runs in a fresh child process (this file, run as a
script) and the parent compares what the two wrote -- with array_equal, and the tracker's outputs with the oracle as well."""
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

# (width, height): the benchmark's size and a small odd one
SIZES = [(1241, 376), (131, 97)]
# shifts of the second image: nearly every iteration stays in its cell / some do / the first steps cross many cells and
# the guess leaves the staged tile (drift radius 5) in the middle of a level
SHIFTS = [(0.2, -0.2), (0.9, 0.9), (6.5, -6.5)]


def _lattice(w, h, step):
    """Every multiple of `step` from two steps outside the image to two steps outside on the other side: the
    reference's lattice (step .. dim - step) plus points whose windows cross or leave every border."""
    xs = np.arange(-2 * step, w + 2 * step + 1, step, dtype=np.float32)
    ys = np.arange(-2 * step, h + 2 * step + 1, step, dtype=np.float32)
    gx, gy = np.meshgrid(xs, ys)
    return np.stack([gx.ravel(), gy.ravel()], 1)


def _mixed(w, h):
    """Lattice points, quarter-pixel points off the lattice and arbitrary fractional points, interleaved in ONE list:
    neighbouring waves of one launch take different paths, and one point takes different paths at different levels."""
    rng = np.random.default_rng(17)
    lat = _lattice(w, h, 10)
    lat = lat[rng.permutation(len(lat))[:300]]
    quarter = (rng.integers(-40, 4 * max(w, h) + 40, (300, 2)) / 4.0).astype(np.float32)
    quarter[:, 0] = np.minimum(quarter[:, 0], w + 10)
    quarter[:, 1] = np.minimum(quarter[:, 1], h + 10)
    integer = rng.integers(-12, [w + 12, h + 12], (200, 2)).astype(np.float32)  # integer, mostly not multiples of 8
    frac = rng.uniform([-12, -12], [w + 12, h + 12], (300, 2)).astype(np.float32)
    pts = np.concatenate([lat, quarter, integer, frac])
    return pts[rng.permutation(len(pts))]


def _lk_cases():
    from ros_stereo_slam_amd import synth

    for (w, h) in SIZES:
        for c in (1, 3):
            a, b = synth.textured_pair(w, h, c, shift=(1.7, -0.6), seed=4 + c)
            for step in (7, 10, 30):
                yield f"lk_{w}x{h}x{c}_step{step}", a, b, _lattice(w, h, step)
            yield f"lk_{w}x{h}x{c}_mixed", a, b, _mixed(w, h)
            for k, shift in enumerate(SHIFTS):
                a, b = synth.textured_pair(w, h, c, shift=shift, seed=11 + 3 * c + k)
                yield f"lk_{w}x{h}x{c}_shift{shift[0]}", a, b, _mixed(w, h)


def _child_lk(out):
    import torch

    torch.cuda.is_available()
    from ros_stereo_slam_amd import capi

    ctx = capi.Context(0)
    res = {}
    for name, a, b, pts in _lk_cases():
        h, w, c = a.shape
        pa, pb = ctx.pyramid(w, h, c).build(a), ctx.pyramid(w, h, c).build(b)
        o, st, err, me = ctx.lk_track(pa, pb, pts)
        res[name + "/out"], res[name + "/st"], res[name + "/err"], res[name + "/me"] = o.view(np.uint32), st, err.view(np.uint32), me.view(np.uint32)
        pa.close()
        pb.close()
    ctx.close()
    np.savez(out, **res)


def _child_frontend(out):
    """The benchmark's stream and shape (grid step 10, 4096 kept, keyframe below 2000 inliers): lock-step groups
    (front-ends that share a context, svo_vo_run_chunks) and the pipelined one-chunk runner.  Their tracking launches
    carry no err pointer: the kernel variant without the level-0 residual."""
    import torch

    from ros_stereo_slam_amd import capi, synth

    n = 31
    poses = synth.loop_trajectory(n, **synth.BENCH_LOOP)
    lefts, rights = synth.stereo_torch(synth.bench_scene(), poses, device="cuda", batch=8)
    torch.cuda.synchronize()
    kw = dict(grid_step=10, anms_keep=4096, keyframe_min_inliers=2000, seed=20261003)
    res = {}
    shared = capi.Context(0)
    bounds = [(0, 11), (10, 21), (20, 31)]
    vos = [capi.VisualOdometry(shared, 1241, 376, 3, **kw) for _ in bounds]
    jobs = []
    for v, (s, e) in zip(vos, bounds):
        v.init(lefts[s], rights[s])
        jobs.append((v, list(lefts[s + 1:e]), list(rights[s + 1:e])))
    for k, (r, v) in enumerate(zip(capi.run_chunks(jobs), vos)):
        assert r[0] == 0 and r[1] == 10
        for i, x in enumerate(r[2:]):
            res[f"lockstep{k}/{i}"] = np.asarray(x)
        res[f"lockstep{k}/ref2"], res[f"lockstep{k}/ref3"] = v.reference()
        v.close()
    shared.close()
    ctx = capi.Context(0)
    v = capi.VisualOdometry(ctx, 1241, 376, 3, **kw)
    v.init(lefts[0], rights[0])
    at = 1
    for k, m in enumerate((1, 2, 7, 3, 17)):  # pieces: the pipeline hands its state over between runs
        r = v.run_chunk(list(lefts[at:at + m]), list(rights[at:at + m]), pipeline=True)
        assert r[0] == 0 and r[1] == m
        for i, x in enumerate(r[2:]):
            res[f"pipe{k}/{i}"] = np.asarray(x)
        at += m
    res["pipe/ref2"], res["pipe/ref3"] = v.reference()
    v.close()
    ctx.close()
    np.savez(out, **res)


def _run_child(what, cache, tmp_path):
    out = tmp_path / f"{what}_{cache}.npz"
    env = dict(os.environ, SVO_LK_CELL_CACHE=str(cache))
    r = subprocess.run([sys.executable, __file__, what, str(out)], env=env, capture_output=True, text=True, timeout=900,
                       cwd=str(ROOT))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return dict(np.load(out))


def _assert_same(a, b):
    assert sorted(a) == sorted(b)
    for k in sorted(a):
        assert np.array_equal(a[k], b[k]), f"{k} differs between SVO_LK_CELL_CACHE=1 and =0"


def test_lk_outputs_equal_with_and_without_the_cell_cache_and_equal_to_the_oracle(orc, tmp_path):
    on, off = _run_child("lk", 1, tmp_path), _run_child("lk", 0, tmp_path)
    _assert_same(on, off)
    orc.set_num_threads(16)
    tracked = 0
    for name, a, b, pts in _lk_cases():
        ro, rs, re, rm = orc.lk_track(a, b, pts)
        assert np.array_equal(on[name + "/st"], rs), name
        assert np.array_equal(on[name + "/me"], np.ascontiguousarray(rm, np.float32).view(np.uint32)), name
        assert np.array_equal(on[name + "/out"], np.ascontiguousarray(ro, np.float32).view(np.uint32)), name
        assert np.array_equal(on[name + "/err"], np.ascontiguousarray(re, np.float32).view(np.uint32)), name
        tracked += int(rs.sum())
        assert rs.any() and not rs.all(), f"{name}: the case should hold tracked points and points that leave the image"
    assert tracked > 5000


def test_frontend_lock_step_and_pipelined_equal_with_and_without_the_cell_cache(tmp_path):
    on, off = _run_child("frontend", 1, tmp_path), _run_child("frontend", 0, tmp_path)
    _assert_same(on, off)
    # the stretch holds keyframe -> non-keyframe -> keyframe transitions in both runners (output 4 of a run: keyframe flags)
    for prefix, parts in (("lockstep", 3), ("pipe", 5)):
        kf = np.concatenate([np.asarray(on[f"{prefix}{k}/4"]).astype(bool).ravel() for k in range(parts)])
        flips = np.count_nonzero(kf[1:] != kf[:-1])
        assert flips >= 2, f"{prefix}: keyframe flags {kf.astype(int)}"


if __name__ == "__main__":
    {"lk": _child_lk, "frontend": _child_frontend}[sys.argv[1]](sys.argv[2])
