"""svo_ba_window on the GPU against the float64 restatement (tests/ba_window_numpy.py, itself held to a dense LM on the CPU by
tests/test_ba_window_numpy.py) with the tolerances tests/test_oracle_ba.py sets between two summation orders, at every seam of the
kernels of csrc/ba_window.hip: point counts around the wavefront, the workgroup and the slab sizes, 1 .. 16 free poses with and
without held ones, runs of one, two and all poses in one window, mono / stereo / mixed, unobserved points at both ends; bit-identity
between runs, contexts and memory modes; the refusals; KeyframeWindow on the rendered scene; the adaptor's smoke program."""
import pathlib
import subprocess

import numpy as np
import pytest

import ba_window_fixtures as F
import ba_window_numpy as M
from ba_fixtures import K4 as K4_ONE, problem
from ros_stereo_slam_amd import capi

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parents[1]


def run_gpu(ctx, w, p, **kw):
    return ctx.ba_window(*F.args(w), params={k: p[k] for k in M.DEFAULTS}, **kw)


def compare(ctx, w, p):
    Pg, Xg, cg, ig = run_gpu(ctx, w, p)
    Pn, Xn, cn, inn = M.ba_window(*F.args(w), p)
    dev = F.check_close(Pg, Xg, ig, Pn, Xn, inn, pytest.approx)
    assert ig["observations"] == inn["observations"] == len(cg)
    assert cg == pytest.approx(cn, rel=1e-6, abs=1e-9)
    if p["huber_mono"] == 0 and p["huber_stereo"] == 0:
        assert cg.sum() == pytest.approx(ig["chi2_after"], rel=1e-12)
    assert np.array_equal(Pg[w["fixed"] == 1], w["poses"][w["fixed"] == 1])
    for i in np.flatnonzero(np.diff(w["obs_start"]) == 0):
        assert np.array_equal(Xg[i], w["pts3d"][i].astype(np.float64))
    return Pg, Xg, cg, ig, dev


@pytest.mark.parametrize("name", list(F.CASES))
def test_named_cases_follow_the_restatement(ctx, name):
    """The cases on which the restatement and the dense LM agree on the CPU: a rejected trial, Huber, free and held gauges."""
    w, p = F.case(name)
    Pg, Xg, cg, ig, dev = compare(ctx, w, p)
    print(name, dev, ig)
    if name in F.ANCHORED:
        free = np.flatnonzero(w["fixed"] == 0)
        e0 = np.linalg.norm(w["poses"][free, 9:] - w["truth"][free, 9:], axis=1)
        assert (np.linalg.norm(Pg[free, 9:] - w["truth"][free, 9:], axis=1) < 0.5 * e0).all()
        assert ig["chi2_after"] > 1e-3 * ig["chi2_before"]


@pytest.mark.parametrize("n", sorted({1, 63, 64, 65, 255, 256, 257, 1025, *F.SLAB_N}))
def test_point_count_seams(ctx, n):
    """Three poses, one held; runs of all, two and one pose in turn; an unobserved point at the first and at the last index."""
    unobserved = (0, n - 1) if n >= 8 else ()
    w = F.window(n=n, n_poses=3, seed=n, unobserved=unobserved, pattern="all" if n < 8 else "all12")
    if n < 3:   # a pose sees a point once, a free pose needs three observations: such a window can only be refused
        with pytest.raises(capi.SvoError, match="fewer than three"):
            run_gpu(ctx, w, F.prm(iterations=3))
        w = F.window(n=n, n_poses=3, seed=n, fixed=(0, 1, 2), pattern="all")
        with pytest.raises(capi.SvoError, match="no free pose"):
            run_gpu(ctx, w, F.prm(iterations=3))
        return
    compare(ctx, w, F.prm(iterations=3))


@pytest.mark.parametrize("free,held", [(1, 0), (2, 0), (3, 0), (16, 0), (16, 16), (1, 1), (3, 2)])
def test_pose_count_seams(ctx, free, held):
    """Held poses first and last around the free ones (16 + 16: the largest window); stereo everywhere fixes the free gauges."""
    n_poses = free + held
    fixed = tuple(range(0, held // 2)) + tuple(range(n_poses - (held - held // 2), n_poses))
    w = F.window(n=70, n_poses=n_poses, seed=100 + n_poses, fixed=fixed, obs="stereo", stride=min(1.0, 4.0 / n_poses))
    assert (np.diff(w["obs_start"]) == n_poses).any() and (np.diff(w["obs_start"]) == 1).any()
    compare(ctx, w, F.prm(iterations=3))


@pytest.mark.parametrize("obs", ["mono", "stereo", "mixed"])
@pytest.mark.parametrize("iterations", [0, 1, 6])
def test_observation_kinds_and_iteration_counts(ctx, obs, iterations):
    w = F.window(n=65, n_poses=4, seed=21, obs=obs)
    Pg, Xg, cg, ig, _ = compare(ctx, w, F.prm(iterations=iterations))
    if iterations == 0:   # nothing moves, bit for bit
        assert np.array_equal(Pg, w["poses"]) and np.array_equal(Xg, w["pts3d"].astype(np.float64))
        assert ig["trials"] == 0 and ig["chi2_before"] == ig["chi2_after"] and ig["lambda_final"] == 0


@pytest.mark.parametrize("n", [5, 440])
def test_one_pose_is_svo_ba_3d2d(ctx, n):
    uv, X, R0, t0, _ = problem(n, 3 if n == 440 else 1, noise=0.2)
    p = M.params(fx=K4_ONE[0], fy=K4_ONE[0], cx=K4_ONE[2], cy=K4_ONE[3], iterations=6)
    uvr = np.c_[uv, np.full(n, np.nan, np.float32)].astype(np.float32)
    Pg, Xg, _, ig = ctx.ba_window(np.r_[R0.ravel(), t0][None], [0], X, np.arange(n + 1), np.zeros(n, np.int32), uvr, params=p)
    t, R, Xo, io = ctx.ba_3d2d(uv, X, K4_ONE, R0, t0, iterations=6)
    F.check_close(Pg, Xg, ig, np.r_[R.ravel(), t][None], Xo, io, pytest.approx)


def test_runs_contexts_and_memory_modes_give_the_same_bits(ctx):
    import torch

    w, p = F.window(n=257, n_poses=5, seed=33, unobserved=(0, 256)), F.prm(iterations=4, huber_mono=F.HUBER_MONO, huber_stereo=F.HUBER_STEREO)
    first = run_gpu(ctx, w, p)
    other = capi.Context(0)
    try:
        for k in range(4):   # five runs in all, the two contexts taking turns
            again = run_gpu(other if k % 2 == 0 else ctx, w, p)
            assert all(np.array_equal(a, b) for a, b in zip(first[:3], again[:3])) and first[3] == again[3]
    finally:
        other.close()
    # device memory, every array between sentinel guard bands
    guard, dev = 64, {}
    for key, arr in (("pts3d", w["pts3d"]), ("obs_start", w["obs_start"]), ("obs_pose", w["obs_pose"]), ("obs_uvr", w["obs_uvr"])):
        flat = np.ascontiguousarray(arr).reshape(-1)
        sentinel = np.full(guard, 0x5A5A5A5A, np.uint32).view(flat.dtype)
        dev[key] = (torch.from_numpy(np.r_[sentinel, flat, sentinel]).cuda(), flat, sentinel)
    view = {k: t[guard:guard + len(f)] for k, (t, f, _) in dev.items()}
    got = ctx.ba_window(w["poses"], w["fixed"], view["pts3d"].view(-1, 3), view["obs_start"], view["obs_pose"], view["obs_uvr"].view(-1, 3),
                        params={k: p[k] for k in M.DEFAULTS}, mem=capi.MEM_DEVICE)
    assert all(np.array_equal(a, b) for a, b in zip(first[:3], got[:3])) and first[3] == got[3]
    for k, (t, f, s) in dev.items():
        back = t.cpu().numpy()
        assert back[:guard].tobytes() == s.tobytes() and back[-guard:].tobytes() == s.tobytes() and back[guard:-guard].tobytes() == f.tobytes()


def test_neighbours_on_the_context_are_undisturbed(ctx):
    uv, X, R0, t0, _ = problem(300, 4)
    ba0 = ctx.ba_3d2d(uv, X, K4_ONE, R0, t0)
    pnp0 = ctx.pnp_ransac(X, uv, K4_ONE, seed=5)
    w, p = F.case("n40_p4_mixed_fixed")
    run_gpu(ctx, w, p)
    ba1 = ctx.ba_3d2d(uv, X, K4_ONE, R0, t0)
    pnp1 = ctx.pnp_ransac(X, uv, K4_ONE, seed=5)
    assert all(np.array_equal(a, b) for a, b in zip(ba0[:3], ba1[:3])) and ba0[3] == ba1[3]
    assert pnp0[0] == pnp1[0] and all(np.array_equal(a, b) for a, b in zip(pnp0[1:4], pnp1[1:4]))


def test_refusals_touch_nothing_with_a_live_context(ctx):
    import test_ba_window_abi as abi

    for name, (mutate, word) in abi.refusals().items():
        a = abi.base_args()
        if name == "starved_pose":
            a["obs_start"], a["obs_pose"], a["obs_uvr"] = abi.STARVED
            a["n_points"], a["pts3d"] = 4, np.ascontiguousarray(a["pts3d"][:4])
        else:
            mutate(a)
        before = None if a["poses"] is None else a["poses"].copy()
        outs = abi.fresh_outputs(a)
        rc = abi.call(ctx.lib, ctx._h, a, outs)
        assert rc == capi.SVO_ERR_ARG and word in ctx.lib.svo_last_error().decode(), name
        assert all((o == 7.25).all() for o in outs), name
        assert before is None or np.array_equal(a["poses"], before), name
    # the same problem, untouched, is accepted
    a = abi.base_args()
    assert abi.call(ctx.lib, ctx._h, a, abi.fresh_outputs(a)) == capi.SVO_OK


def test_keyframe_window_on_the_rendered_scene(ctx):
    from ros_stereo_slam_amd import local_ba, synth

    size, K4, baseline = (640, 240), (360.0, 360.0, 320.0, 120.0), 0.54
    scene = synth.Scene()
    poses = synth.corridor_trajectory(6, step=0.5)
    win = local_ba.KeyframeWindow(ctx, K4, baseline, seed=7, grid_step=20)
    left, right = scene.stereo(*poses[0], K=K4, size=size, baseline=baseline)[:2]
    n = win.open(left, right)
    assert n > 100
    for R, t in poses[1:]:
        assert win.add(scene.stereo(R, t, K=K4, size=size, baseline=baseline)[0]) >= 10
    arrays = win.arrays()
    assert len(arrays[0]) == 6 and arrays[1].tolist() == [1, 0, 0, 0, 0, 0] and arrays[3][-1] == len(arrays[4])
    assert (np.diff(arrays[3]) >= 1).all() and (np.diff(arrays[3]) <= 6).all()   # every point has its keyframe observation
    Pg, Xg, cg, ig = win.adjust()
    direct = ctx.ba_window(*arrays, params=dict(fx=K4[0], fy=K4[1], cx=K4[2], cy=K4[3], bf=K4[0] * baseline))
    assert all(np.array_equal(a, b) for a, b in zip((Pg, Xg, cg), direct[:3])) and ig == direct[3]
    assert ig["chi2_after"] < ig["chi2_before"] and ig["observations"] == len(arrays[4])
    assert np.array_equal(Pg[0], np.r_[np.eye(3).ravel(), np.zeros(3)])


def test_smoke_program_is_the_python_path(ctx, tmp_path):
    import test_ba_window_abi as abi

    exe = tmp_path / "ba_window_smoke"
    abi.build_smoke(exe)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "ba window smoke ok" in out.stdout, (out.stdout, out.stderr)
    w, p = F.case("n40_p4_mixed_fixed_huber")
    hx = lambda v: float(v).hex()
    lines = [f"{len(w['poses'])} {len(w['pts3d'])} {len(w['obs_pose'])} {p['iterations']}",
             " ".join(hx(p[k]) for k in ("fx", "fy", "cx", "cy", "bf", "huber_mono", "huber_stereo"))]
    lines += [" ".join(hx(v) for v in P) + f" {int(f)}" for P, f in zip(w["poses"], w["fixed"])]
    lines += [" ".join(hx(v) for v in X) for X in w["pts3d"]]
    lines += [" ".join(str(int(s)) for s in w["obs_start"])]
    lines += [f"{int(j)} " + " ".join(hx(v) for v in z) for j, z in zip(w["obs_pose"], w["obs_uvr"])]
    (tmp_path / "window.txt").write_text("\n".join(lines) + "\n")
    out = subprocess.run([str(exe), str(tmp_path / "window.txt")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "ba window smoke ok" in out.stdout, (out.stdout, out.stderr)
    Pg, _, _, ig = run_gpu(ctx, w, p)
    rows = [l.split() for l in out.stdout.splitlines()]
    got = np.array([[float.fromhex(v) for v in r[2:]] for r in rows if r[0] == "pose"])
    info = [float.fromhex(v) for r in rows if r[0] == "info" for v in r[1:]]
    assert np.array_equal(got, Pg)
    assert info == [ig["chi2_before"], ig["chi2_after"], ig["lambda_final"], ig["iterations"], ig["trials"], ig["observations"]]
