"""Pins the oracle's two-view geometry restatement (reference call sites
src/tracking.cpp:34,75; src/triangulation.cpp:142-160; src/keyFrameManagement.cpp:20-30;
src/VisualSLAM.cpp:70-74) with analytic known answers and numpy/scipy cross-checks."""
import numpy as np
import pytest
from scipy.spatial.transform import Rotation as Rot

from core_numpy import triangulate as numpy_dlt
from geom_fixtures import BASELINE, K, K4, project, scene_points, two_view


def test_rng_is_counter_based(orc):
    a = [orc.rng_u32(7, i, d) for i in range(4) for d in range(4)]
    assert len(set(a)) == 16
    assert orc.rng_u32(7, 2, 3) == a[2 * 4 + 3]
    assert orc.rng_u32(8, 2, 3) != a[2 * 4 + 3]


def test_seven_point_contains_true_F(orc):
    x1, x2, gt, X, R, t = two_view(n=50, n_out=0)
    Fs = orc.seven_point(x1[:7].astype(np.float64), x2[:7].astype(np.float64))
    assert 1 <= len(Fs) <= 3
    h1, h2 = np.c_[x1, np.ones(50)], np.c_[x2, np.ones(50)]
    alg = [np.abs(np.einsum("ni,ij,nj->n", h2, F, h1)) for F in Fs]
    # every model interpolates the 7 sample points; one of them explains all 50
    for a, F in zip(alg, Fs):
        assert a[:7].max() < 1e-9
        assert abs(np.linalg.det(F)) < 1e-12
        assert abs(np.linalg.norm(F) - 1) < 1e-12
    assert min(np.median(a) for a in alg) < 1e-4  # float32 pixel coordinates


def test_f_error_matches_numpy(orc):
    x1, x2, *_ = two_view(n=30, n_out=5)
    F = orc.seven_point(x1[:7].astype(np.float64), x2[:7].astype(np.float64))[0]
    got = orc.f_error(F, x1, x2)
    h1, h2 = np.c_[x1, np.ones(30)].astype(np.float64), np.c_[x2, np.ones(30)].astype(np.float64)
    l2, l1 = h1 @ F.T, h2 @ F
    d2 = np.einsum("ni,ni->n", h2, l2) ** 2 / (l2[:, 0] ** 2 + l2[:, 1] ** 2)
    d1 = np.einsum("ni,ni->n", h1, l1) ** 2 / (l1[:, 0] ** 2 + l1[:, 1] ** 2)
    assert np.allclose(got, np.maximum(d1, d2).astype(np.float32), rtol=1e-5)


@pytest.mark.parametrize("thr", [1.0, 3.0])
@pytest.mark.parametrize("seed", [1, 42])
def test_fransac_finds_ground_truth_inliers(orc, thr, seed):
    x1, x2, gt, X, R, t = two_view(n=400, n_out=80, seed=seed, noise=0.1)
    cnt, mask, F, iters = orc.fransac(x1, x2, thr, seed=seed)
    m = mask.astype(bool)
    assert cnt == m.sum()
    assert (m & gt).sum() >= 0.94 * gt.sum()          # minimal-sample model, no refit: most true inliers kept
    assert (m & ~gt).sum() <= 6                        # outliers survive only near their epipolar line
    assert iters < 200                                 # adaptive stop (80% inliers -> ~20 iterations)
    assert abs(np.linalg.det(F)) < 1e-10


def test_fransac_is_deterministic_and_seeded(orc):
    x1, x2, *_ = two_view(n=300, n_out=100, seed=5, noise=0.2)
    a = orc.fransac(x1, x2, 1.0, seed=9)
    b = orc.fransac(x1, x2, 1.0, seed=9)
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[3] == b[3]


def test_fransac_degenerate_inputs(orc):
    x1, x2, *_ = two_view(n=6, n_out=0)
    cnt, mask, F, iters = orc.fransac(x1, x2, 1.0)
    assert cnt == 0 and mask.sum() == 0
    cnt, mask, F, iters = orc.fransac(np.zeros((0, 2)), np.zeros((0, 2)), 1.0)
    assert cnt == 0


def test_triangulate_known_answer_and_numpy_dlt(orc):
    P1, P2 = orc.stereo_projections(*K4, BASELINE)
    assert np.allclose(P1, K @ np.c_[np.eye(3), np.zeros(3)])
    assert np.allclose(P2, K @ np.c_[np.eye(3), [-BASELINE, 0, 0]])
    X = scene_points(300, 3)
    a = project(X).astype(np.float32)
    b = project(X, np.eye(3), np.array([-BASELINE, 0, 0])).astype(np.float32)
    xyz, h = orc.triangulate(P1, P2, a, b)
    assert (np.linalg.norm(xyz - X, axis=1) / np.linalg.norm(X, axis=1)).max() < 3e-3  # float32 pixels
    # noisy case (rays do not meet): compare with numpy's SVD-based DLT
    rng = np.random.default_rng(0)
    b2 = (b + rng.normal(0, 0.5, b.shape)).astype(np.float32)
    xyz2, h2 = orc.triangulate(P1, P2, a, b2)
    pick = np.arange(0, 300, 17)
    ref, vs = numpy_dlt(P1, P2, a[pick], b2[pick])      # the float64 SVD DLT of tests/core_numpy.py
    for i, r, v in zip(pick, ref, vs):
        assert np.allclose(xyz2[i], r, rtol=2e-4, atol=1e-4)
        assert abs(abs(np.dot(h2[i].astype(np.float64), v)) - 1) < 1e-5  # same direction, sign free


def test_transform_points_float_double_mix(orc):
    rng = np.random.default_rng(1)
    Rt = np.c_[Rot.from_rotvec([0.2, -0.1, 0.3]).as_matrix(), [1.5, -0.2, 10.0]]
    pts = rng.uniform(-20, 20, (100, 3)).astype(np.float32)
    got = orc.transform_points(Rt, pts)
    ref = (pts.astype(np.float64) @ Rt[:, :3].T + Rt[:, 3]).astype(np.float32)
    assert np.abs(got - ref).max() <= 4e-6 * 40  # a few float32 ulps at |x| ~ 40
    assert got.dtype == np.float32


def test_get_colors(orc):
    rng = np.random.default_rng(2)
    img = rng.integers(0, 256, (40, 60, 3), dtype=np.uint8)
    xy = np.array([[0.0, 0.0], [59.9, 39.9], [10.7, 20.2]], np.float32)
    got = orc.get_colors(img, xy)
    assert np.array_equal(got, np.array([img[0, 0], img[39, 59], img[20, 10]], np.float32))


def test_rodrigues_matches_scipy(orc):
    rng = np.random.default_rng(3)
    for _ in range(50):
        r = rng.normal(0, 1, 3)
        r *= rng.uniform(0, 3.0) / np.linalg.norm(r)
        R = orc.rodrigues(r)
        assert np.abs(R - Rot.from_rotvec(r).as_matrix()).max() < 1e-14
        assert np.abs(orc.rodrigues_inv(R) - r).max() < 1e-9
    assert np.array_equal(orc.rodrigues(np.zeros(3)), np.eye(3))


def test_compose_camera_pose(orc):
    r, t = np.array([0.1, -0.2, 0.05]), np.array([0.3, -0.1, 2.0])
    R, c = orc.compose_camera_pose(r, t)
    Rm = Rot.from_rotvec(r).as_matrix()
    assert np.allclose(R, Rm.T, atol=1e-15) and np.allclose(c, -Rm.T @ t, atol=1e-15)
