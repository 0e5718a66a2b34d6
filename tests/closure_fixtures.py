"""The image pair of the loop-closure measurement tests: rendered once per test session, shared by the tests that need it."""
import numpy as np

from ros_stereo_slam_amd import capi, synth

SIZE = (640, 240)
K4 = (360.0, 360.0, 320.0, 120.0)
SEED = 11


def quat_of(R):
    """include/svo.h's formula, operation by operation (numpy float64 scalars: IEEE, as the library's host code)"""
    R = np.asarray(R, np.float64).reshape(9)
    one, two, four = np.float64(1), np.float64(2), np.float64(4)
    tr = R[0] + R[4] + R[8]
    if tr > 0:
        s = two * np.sqrt(tr + one)
        q = [(R[7] - R[5]) / s, (R[2] - R[6]) / s, (R[3] - R[1]) / s, s / four]
    elif R[0] > R[4] and R[0] > R[8]:
        s = two * np.sqrt(one + R[0] - R[4] - R[8])
        q = [s / four, (R[1] + R[3]) / s, (R[2] + R[6]) / s, (R[7] - R[5]) / s]
    elif R[4] > R[8]:
        s = two * np.sqrt(one + R[4] - R[0] - R[8])
        q = [(R[1] + R[3]) / s, s / four, (R[5] + R[7]) / s, (R[2] - R[6]) / s]
    else:
        s = two * np.sqrt(one + R[8] - R[0] - R[4])
        q = [(R[2] + R[6]) / s, (R[5] + R[7]) / s, s / four, (R[3] - R[1]) / s]
    nrm = np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    sgn = np.float64(-1.0 if q[3] / nrm < 0 else 1.0)
    return np.array([sgn * (x / nrm) for x in q])


_PAIR = None


def make_pair(ctx):
    """One corridor view with its stereo partner (the newest frame: grid points, 3-D from svo_triangulate in its camera
    frame) and the view of a camera 0.3 m further and 2 degrees turned (the matched frame); the true relative pose."""
    global _PAIR
    if _PAIR is not None:
        return _PAIR
    scene = synth.Scene()
    Ra, ta = np.eye(3), np.array([0.1, 0.0, 3.0])
    Rb, tb = synth.rot_y(np.deg2rad(2.0)), ta + np.array([0.0, 0.0, 0.3])
    left, right, _ = scene.stereo(Ra, ta, K=K4, size=SIZE, channels=1)
    matched, _ = scene.render(Rb, tb, K=K4, size=SIZE, channels=1)
    w, h = SIZE
    grid = ctx.grid_keypoints(h, w, 20)
    pl, pr = ctx.pyramid(w, h, 1).build(left), ctx.pyramid(w, h, 1).build(right)
    nxt, st, _, _ = ctx.lk_track(pl, pr, grid)
    P1, P2 = capi.stereo_projections(*K4, synth.KITTI_BASELINE)
    xyz, _ = ctx.triangulate(P1, P2, grid, nxt)
    ok = (st == 1) & np.isfinite(xyz).all(axis=1) & (xyz[:, 2] > 0.5) & (xyz[:, 2] < 60.0)
    pl.close()
    pr.close()
    true = np.r_[Ra.T @ (tb - ta), quat_of(Ra.T @ Rb)]
    _PAIR = dict(newest=left, matched=matched, xy=np.ascontiguousarray(grid[ok]), xyz=np.ascontiguousarray(xyz[ok]), true=true)
    return _PAIR
