"""svo_homography_4pt / svo_find_homography / svo_homography_pose on the MI355X against tests/homography_numpy.py, and
StereoProcess::monocularTriangulate with HOMOGRAPHY_FLAG end to end on two rendered frames of a textured plane (the Python
composition, the C++ adaptor and the generator's truth)."""
import ctypes as C
import subprocess
import time

import numpy as np
import pytest

import homography_numpy as hn
from test_homography_abi import build_smoke
from test_homography_numpy import (D_SENSITIVITY, K4, NOISES, OUTLIERS, SEEDS, SIZES, equality_fixture, four_point_samples,
                                   plane_problem, pose_fixture, transfer, unit_h)

pytestmark = pytest.mark.gpu

H_BOUND = max(16 * D_SENSITIVITY, 1e-12)


def test_minimal_solver(ctx):
    x1, x2 = four_point_samples(2000, seed=11)
    H, ok = ctx.homography_4pt(x1, x2)
    rH, rok = hn.solve_4pt(x1, x2)
    assert np.array_equal(ok != 0, rok) and 1500 <= rok.sum() < 2000
    assert np.all(H[~rok] == 0) and np.all(H[rok, 2, 2] == 1)
    worst = max(np.abs(transfer(H[k], x1[k]) - transfer(rH[k], x1[k])).max() for k in np.flatnonzero(rok))
    print(f"svo_homography_4pt against the restatement: largest transfer difference {worst:.3e} px, "
          f"{int(np.sum(np.all(H.reshape(-1, 9) == rH, 1)))} of 2000 with equal bits")
    assert worst <= 1e-9


@pytest.mark.parametrize("n", SIZES)
def test_ransac_equals_the_restatement(ctx, n):
    worst = 0.0
    for outliers in OUTLIERS:
        for noise in NOISES:
            for seed in SEEDS:
                case = (n, outliers, noise, seed)
                p1, p2, r = equality_fixture(*case)
                assert r.margin_ok, ("fixture too close to the threshold for an equality test", case)
                H, mask, count, iters = ctx.find_homography(p1, p2, seed=seed)
                assert np.array_equal(mask, r.mask) and count == r.count and iters == r.iters, case
                if r.count == 0:
                    assert not H.any(), case
                    continue
                diff = np.abs(unit_h(H) - unit_h(r.H)).max()
                worst = max(worst, diff)
                assert diff <= H_BOUND, (case, diff)
    print(f"n = {n}: largest difference of the unit-norm H {worst:.3e} (bound {H_BOUND:.3e})")


def test_degenerate_input_ends_with_no_model(ctx):
    line = np.c_[np.linspace(10, 900, 500), np.linspace(20, 300, 500)].astype(np.float32)
    same = np.full((500, 2), 7, np.float32)
    three = np.array([[0, 0], [5, 5], [10, 10], [3, 9]], np.float32)
    for a, b in ((line, line + 2), (same, same + 2), (three, three)):
        t0 = time.perf_counter()
        H, mask, count, iters = ctx.find_homography(a, b, max_iters=20000)
        dt = time.perf_counter() - t0
        r = hn.find_homography(a, b, max_iters=64)
        assert count == 0 == r.count and not mask.any() and not H.any()
        assert dt < 2.0, dt                                   # every sample loop is bounded: 20000 rejected iterations, at once


def guarded(lib, ctx, P1, P2, seed):
    """svo_find_homography on host arrays with guard bands around every output -> the outputs"""
    sizes = [len(p) for p in P1]
    offsets = np.ascontiguousarray(np.r_[0, np.cumsum(sizes)], np.int32)
    total, k, G = int(offsets[-1]), len(P1), 64
    a, b = np.ascontiguousarray(np.concatenate(P1)), np.ascontiguousarray(np.concatenate(P2))
    mask, H, cnt, its = (np.full(total + 2 * G, 0xA5, np.uint8), np.full(9 * k + 2 * G, -7.5), np.full(k + 2 * G, -9, np.int32),
                         np.full(k + 2 * G, -9, np.int32))
    ptr = lambda v, item: C.c_void_p(v.ctypes.data + G * item)  # noqa: E731
    rc = lib.svo_find_homography(ctx._h, a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), offsets.ctypes.data_as(C.c_void_p),
                                 k, C.c_double(3.0), C.c_double(0.995), 2000, C.c_uint64(seed), ptr(mask, 1), ptr(H, 8), ptr(cnt, 4),
                                 ptr(its, 4), 0)
    assert rc == 0
    for v, fill in ((mask, 0xA5), (H, -7.5), (cnt, -9), (its, -9)):
        assert (v[:G] == fill).all() and (v[-G:] == fill).all()
    return mask[G:-G], H[G:-G].reshape(k, 3, 3), cnt[G:-G], its[G:-G], offsets


def test_batch_device_and_determinism(ctx):
    import torch

    from ros_stereo_slam_amd import capi

    sizes = [5, 4, 9, 40, 300, 2000, 3, 1200, 77, 500, 16, 8000, 250, 31, 1000, 64]
    probs = [plane_problem(n, 0.3 + 0.02 * k, seed=50 + k, noise=0.3) for k, n in enumerate(sizes)]
    P1, P2 = [p[0] for p in probs], [p[1] for p in probs]
    batch = ctx.find_homography(P1, P2, seed=9)
    again = ctx.find_homography(P1, P2, seed=9)
    other = capi.Context(0)
    try:
        for k in range(16):
            one = (ctx if k % 2 else other).find_homography(P1[k], P2[k], seed=9)     # two contexts taking turns
            for x, y, z in zip(batch[k], one, again[k]):
                assert np.array_equal(np.asarray(x), np.asarray(y)) and np.array_equal(np.asarray(x), np.asarray(z)), k
    finally:
        other.close()
    assert batch[1][2] == 4 and batch[6][2] == 0 and all(batch[k][2] > 4 for k in (3, 5, 11, 15))
    dev = ctx.find_homography([torch.from_numpy(a).cuda() for a in P1], [torch.from_numpy(b).cuda() for b in P2], seed=9)
    for k in range(16):
        assert np.array_equal(dev[k][0], batch[k][0]) and np.array_equal(dev[k][1].cpu().numpy(), batch[k][1])
        assert dev[k][2:] == batch[k][2:]
    mask, H, cnt, its, offsets = guarded(ctx.lib, ctx, P1, P2, seed=9)
    for k in range(16):
        assert np.array_equal(H[k], batch[k][0]) and np.array_equal(mask[offsets[k]:offsets[k + 1]], batch[k][1])
        assert (cnt[k], its[k]) == batch[k][2:]


def test_pose_equals_the_restatement(ctx):
    cases = []
    for normal, t in (((0.5, 0.1, 1.0), (0.6, -0.1, 0.4)), ((0.0, 0.0, 1.0), (0.1, 0.0, 0.5)), ((0.1, -0.25, 1.0), (0.0, 0.3, -0.4))):
        p1, p2, R, tt, nn, d = pose_fixture(normal, t=t, n=300 + 64 * len(cases) + 1)
        cases.append((hn.homography_from_pose(R, tt, nn, d, K4), p1, p2))
    rng = np.random.default_rng(3)
    singles = []
    for H, p1, p2 in cases:
        for mask in (None, (rng.random(len(p1)) < 0.8).astype(np.uint8)):
            got = ctx.homography_pose(H, p1, p2, K4, mask=mask)
            want = hn.homography_pose(H, p1, p2, K4, mask=mask)
            for x, y in zip(got, want):
                assert np.array_equal(np.asarray(x), np.asarray(y))
            if mask is not None:
                assert not (got[4] & (mask == 0)).any() and 0 < got[4].sum() < len(p1)
            else:
                singles.append(got)
    assert singles[1][3][0] == singles[1][3][2] == len(cases[1][1])          # the head-on tie shows in good4
    batch = ctx.homography_pose([c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases], K4)
    for got, one in zip(batch, singles):
        for x, y in zip(got, one):
            assert np.array_equal(np.asarray(x), np.asarray(y))
    R, t, n, good4, mask = ctx.homography_pose(np.zeros((3, 3)), cases[0][1], cases[0][2], K4)    # a singular H: zeros
    assert not R.any() and not t.any() and not n.any() and good4 == [0, 0, 0, 0] and not mask.any()
    # the pure rotation: one candidate, t = 0 (its triangulation has no baseline, so its count says nothing)
    p1, p2, R0, tt, nn, d = pose_fixture((0.0, 0.0, 1.0), t=(0.0, 0.0, 0.0))
    H = hn.homography_from_pose(R0, tt, nn, d, K4)
    R, t, n, good4, mask = ctx.homography_pose(H, p1, p2, K4)
    (Rn, tn, n_n), = hn.decompose(H, K4)
    assert np.array_equal(R, Rn) and not t.any() and np.array_equal(n, n_n) and good4[1:] == [0, 0, 0]


def test_the_other_two_view_calls_keep_their_bits(ctx):
    from test_gpu_essential import pixel_problem

    p1, p2, *_ = pixel_problem(1500, 0.3, seed=77, noise=0.3)

    def others():
        E, emask, ecount, eiters = ctx.find_essential(p1, p2, K4, seed=4)
        F = ctx.fransac(p1, p2, 3.0, 0.99, 1000, seed=3)
        pose = ctx.recover_pose(E[0], p1, p2, K4)
        return [E, emask, ecount, eiters, *F, *pose]

    before = others()
    q1, q2, _, _ = plane_problem(3000, 0.4, seed=78, noise=0.3)
    H, *_ = ctx.find_homography(q1, q2, seed=1)
    ctx.homography_pose(H, q1, q2, K4)
    for x, y in zip(before, others()):
        assert np.array_equal(np.asarray(x), np.asarray(y))


# ---- end to end: monocularTriangulate with HOMOGRAPHY_FLAG on two rendered frames of a textured plane ----
def mono_python(ctx, im1, im2, K=K4, grid_step=30, seed=0):
    """the adaptor's steps in Python: grid + LK + F-RANSAC (3 px), findHomography (3 px, 0.995, 2000), the planar pose, DLT
    of all F-inliers with P1 = K[I|0], P2 = K[R|t]."""
    h, w, c = im1.shape
    pts = ctx.grid_keypoints(h, w, grid_step)
    pa, pb = ctx.pyramid(w, h, c).build(im1), ctx.pyramid(w, h, c).build(im2)
    trk, status, _, _ = ctx.lk_track(pa, pb, pts)
    pa.close()
    pb.close()
    a, b = ctx.compact(status, pts, trk)
    _, fmask, _, _ = ctx.fransac(a, b, 3.0, 0.99, 1000, seed=seed + 3)
    a, b = ctx.compact(fmask, a, b)
    H, _, count, _ = ctx.find_homography(a, b, seed=seed + 4)
    R, t, n, good4, _ = ctx.homography_pose(H, a, b, K)
    Km = [[K[0], 0.0, K[2]], [0.0, K[1], K[3]], [0.0, 0.0, 1.0]]
    Rt = np.hstack([R, t[:, None]])
    P1 = np.array([[Km[r][c] if c < 3 else 0.0 for c in range(4)] for r in range(3)])
    P2 = np.zeros((3, 4))
    for r in range(3):  # the adaptor's product, in its order
        for c in range(4):
            s = 0.0
            for k in range(3):
                s += Km[r][k] * float(Rt[k, c])
            P2[r, c] = s
    xyz, _ = ctx.triangulate(P1, P2, a, b)
    return a, b, H, R, t, n, good4, xyz


def test_end_to_end_on_a_rendered_plane(ctx, tmp_path):
    import torch

    from ros_stereo_slam_amd import synth

    # one textured plane: the ground alone (the walls out of sight), seen by a camera pitched down at it
    sc = synth.Scene(wall_x=1e6)
    c5, s5 = np.cos(-0.5), np.sin(-0.5)
    R1, t1 = np.array([[1, 0, 0], [0, c5, -s5], [0, s5, c5]]), np.zeros(3)
    R2, t2 = R1 @ synth.rot_y(0.02), np.array([0.5, 0.0, 0.1])
    frames = synth.render_torch(sc, np.stack([R1, R2]), np.stack([t1, t2]), K=K4).cpu().numpy()
    im1, im2 = frames[0], frames[1]
    h, w, _ = im1.shape
    a, b, H, R, t, n, good4, xyz = mono_python(ctx, im1, im2)
    (tmp_path / "f1").write_bytes(im1.tobytes())
    (tmp_path / "f2").write_bytes(im2.tobytes())
    exe = tmp_path / "homography_mono_smoke"
    build_smoke(exe)
    out = subprocess.run([str(exe), str(tmp_path / "f1"), str(tmp_path / "f2"), str(w), str(h), str(tmp_path / "o")],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert np.array_equal(np.fromfile(tmp_path / "o.pts", np.float32).reshape(-1, 4), np.c_[a, b])
    assert np.array_equal(np.fromfile(tmp_path / "o.xyz", np.float32).reshape(-1, 3), xyz)
    pose = np.fromfile(tmp_path / "o.pose", np.float64)
    assert np.array_equal(pose[:9].reshape(3, 3), R) and np.array_equal(pose[9:12], t) and np.array_equal(pose[12:], n)
    # truth: X2 = R_rel X1 + t_rel with camera-in-world poses (R_i, t_i)
    R_rel, t_rel = R2.T @ R1, R2.T @ (t1 - t2)
    ang = lambda Ra, Rb: np.degrees(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1) / 2, -1, 1)))  # noqa: E731
    # the true candidate is the one picked: of the decomposition's rotations and directions, the chosen is the nearest
    sols = hn.decompose(H, K4)
    errs = [ang(s[0], R_rel) + np.degrees(np.arccos(np.clip(hn.unit(s[1]) @ t_rel / np.linalg.norm(t_rel), -1, 1))) for s in sols]
    rot_err = ang(R, R_rel)
    dir_err = np.degrees(np.arccos(np.clip(t @ t_rel / np.linalg.norm(t_rel), -1, 1)))
    print(f"monocularTriangulate with HOMOGRAPHY_FLAG: {len(a)} F-inliers, good4 {good4}, R error {rot_err:.4f} deg, "
          f"t direction error {dir_err:.4f} deg, normal {np.round(n, 4)}")
    assert rot_err + dir_err == min(errs), (errs, good4)
    torch.cuda.synchronize()
