"""tests/homography_numpy.py against independent definitions (CPU only): the 4-point solve against numpy's SVD of the DLT
matrix, checkSubset on hand-made samples, the RANSAC on exact data, the refit and polish on noise-free data, the
decomposition against Hn = R + t n^T, the planar pose, and the summation-order sensitivity of the refit that
tests/test_gpu_homography.py takes its bound from.  The fixtures of the GPU tests are made here."""
import functools

import numpy as np
import pytest

import homography_numpy as hn

K4 = (718.856, 718.856, 607.1928, 185.2157)
W, H_IMG = 1241, 376

# the GPU equality cases (tests/test_gpu_homography.py)
SIZES = [3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 63, 64, 65, 255, 256, 257, 2000]
OUTLIERS = [0.0, 0.3, 0.6]
NOISES = [0.0, 0.5]
SEEDS = [31, 32, 33]
# the largest difference of the unit-norm H between the refit + polish over the inliers in given and in reversed order,
# over every fixture above: measured by test_summation_order_sensitivity, which holds it to this figure
D_SENSITIVITY = 2.1e-7


def rot(r):
    r = np.asarray(r, np.float64)
    th = np.linalg.norm(r)
    if th == 0:
        return np.eye(3)
    k = r / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def project(X):
    return np.c_[K4[0] * X[:, 0] / X[:, 2] + K4[2], K4[1] * X[:, 1] / X[:, 2] + K4[3]]


def plane_points(n, rng, normal, d):
    """n pixels of the frame and their points on the plane normal . X = d (first camera's frame)"""
    p = np.c_[rng.uniform(0, W, n), rng.uniform(0, H_IMG, n)]
    ray = np.c_[(p[:, 0] - K4[2]) / K4[0], (p[:, 1] - K4[3]) / K4[1], np.ones(n)]
    return p, ray * (d / (ray @ normal))[:, None]


def plane_scene(n, seed, normal=(0.1, -0.25, 1.0), d=8.0, R=None, t=None):
    """-> (p1, p2 float64 pixels, R, t, unit normal, d): X2 = R X1 + t"""
    rng = np.random.default_rng(seed)
    normal = np.asarray(normal, np.float64) / np.linalg.norm(normal)
    R = rot(np.array([0.02, -0.05, 0.015]) + rng.normal(size=3) * 0.01) if R is None else R
    t = np.array([0.6, -0.1, 0.4]) + rng.normal(size=3) * 0.05 if t is None else np.asarray(t, np.float64)
    p1, X = plane_points(n, rng, normal, d)
    return p1, project(X @ R.T + t), R, t, normal, d


def plane_problem(n, outlier_frac, seed, noise=0.0):
    """-> (p1, p2 float32, the true mask, the true pixel homography)"""
    p1, p2, R, t, normal, d = plane_scene(n, seed)
    rng = np.random.default_rng(seed + 100000)
    if noise:
        p1 = p1 + rng.normal(size=p1.shape) * noise
        p2 = p2 + rng.normal(size=p2.shape) * noise
    no = int(round(n * outlier_frac))
    rows = rng.permutation(n)[:no]
    ang = rng.uniform(0, 2 * np.pi, no)
    p2[rows] += np.c_[np.cos(ang), np.sin(ang)] * rng.uniform(12, 80, no)[:, None]
    truth = np.ones(n, np.uint8)
    truth[rows] = 0
    return p1.astype(np.float32), p2.astype(np.float32), truth, hn.homography_from_pose(R, t, normal, d, K4)


def transfer(H, p):
    q = np.c_[np.asarray(p, np.float64), np.ones(len(p))] @ np.asarray(H, np.float64).reshape(3, 3).T
    return q[:, :2] / q[:, 2:]


def four_point_samples(count, seed):
    """-> (x1, x2: count x 4 x 2 float64): quadrilaterals under random homographies; every 10th with three collinear
    points in one image, every 10th + 5 with its fourth point carried across a side in image 2"""
    rng = np.random.default_rng(seed)
    x1, x2 = np.zeros((count, 4, 2)), np.zeros((count, 4, 2))
    for k in range(count):
        c = np.array([rng.uniform(200, 1000), rng.uniform(80, 300)])
        w, h = rng.uniform(40, 400), rng.uniform(30, 150)
        q = c + np.array([[-w, -h], [w, -h], [w, h], [-w, h]]) * rng.uniform(0.6, 1.0, (4, 1)) + rng.normal(size=(4, 2)) * 3
        q = q[rng.permutation(4)]
        Hm = np.eye(3) + rng.normal(size=(3, 3)) * np.array([[0.1, 0.1, 30], [0.1, 0.1, 30], [1e-4, 1e-4, 0]])
        Hm[2, 2] = 1
        x1[k], x2[k] = q, transfer(Hm, q)
        if k % 10 == 0:
            which = x1 if k % 20 == 0 else x2
            which[k, 2] = 0.3 * which[k, 0] + 0.7 * which[k, 1]
        elif k % 10 == 5:
            x2[k, 3] = x2[k, 0] + x2[k, 1] - x2[k, 3] + (x2[k, 0] + x2[k, 1] - 2 * x2[k, 2]) * 0.5
    return x1, x2


@functools.lru_cache(maxsize=None)
def equality_fixture(n, outliers, noise, seed):
    """one GPU equality case -> (p1, p2, the restatement's result); the data's seed is a function of the case"""
    p1, p2, _, _ = plane_problem(n, outliers, 7000 + 13 * n + int(outliers * 10) * 3 + int(noise * 2) + seed, noise)
    return p1, p2, hn.find_homography(p1, p2, seed=seed)


def unit_h(H):
    H = np.asarray(H, np.float64).reshape(9)
    return H / np.linalg.norm(H)


# ---- the minimal solve ----
def test_four_point_solve_against_the_svd():
    x1, x2 = four_point_samples(2000, seed=11)
    H, ok = hn.solve_4pt(x1, x2)
    assert 1500 <= ok.sum() < 2000 and np.all(H[~ok] == 0) and np.all(H[ok, 8] == 1)
    worst = 0.0
    for k in np.flatnonzero(ok):
        A = []
        for (X, Y), (x, y) in zip(x1[k], x2[k]):
            A += [[X, Y, 1, 0, 0, 0, -x * X, -x * Y, -x], [0, 0, 0, X, Y, 1, -y * X, -y * Y, -y]]
        A = np.array(A)
        scale = np.abs(A).max(0)  # column scaling: the null vector of the scaled matrix, scaled back
        h = np.linalg.svd(A / scale)[2][-1] / scale
        worst = max(worst, np.abs(transfer(H[k], x1[k]) - transfer(h / h[8], x1[k])).max())
        assert np.abs(transfer(H[k], x1[k]) - x2[k]).max() <= 1e-9
    print(f"4-point solve against the SVD: largest transfer difference {worst:.3e} px")
    assert worst <= 1e-9


def test_check_subset_hand_made_cases():
    sq = np.array([[0.0, 0.0], [10.0, 0.0], [10.0, 10.0], [0.0, 10.0]])
    assert hn.check_subset(sq, sq + 3)                                     # a proper sample
    col = sq.copy()
    col[2] = [20.0, 0.0]                                                   # 0, 1, 2 on one line
    assert not hn.check_subset(col, sq) and not hn.check_subset(sq, col)   # in image 1 only, in image 2 only
    last = sq.copy()
    last[3] = [5.0, 5.0]                                                   # 0, 2, 3 on one line
    assert not hn.check_subset(last, sq)
    cross = sq.copy()
    cross[3] = [5.0, -4.0]                                                 # the fourth point crosses the line 0-1
    assert not hn.check_subset(sq, cross) and not hn.check_subset(cross, sq)
    assert hn.check_subset(cross, cross)
    H, ok = hn.solve_4pt(np.stack([sq, col, sq]), np.stack([sq + 3, sq, cross]))
    assert list(ok) == [True, False, False] and np.all(H[1:] == 0)
    assert np.abs(H[0].reshape(3, 3) - np.array([[1, 0, 3], [0, 1, 3], [0, 0, 1.0]])).max() <= 1e-12


# ---- the loop ----
@pytest.mark.parametrize("outliers", [0.3, 0.6])
def test_ransac_exact_data_returns_the_true_mask(outliers):
    p1, p2, truth, Ht = plane_problem(1500, outliers, seed=21 + int(outliers * 10))
    r = hn.find_homography(p1, p2, seed=5)
    assert np.array_equal(r.mask, truth) and r.count == truth.sum() and 0 < r.iters < 2000
    corners = np.array([[0, 0], [W, 0], [W, H_IMG], [0, H_IMG]], np.float64)
    assert np.abs(transfer(r.H, corners) - transfer(Ht, corners)).max() <= 1e-3   # float pixels: 6e-5 px of rounding


def test_small_problems_and_degenerate_input():
    p1, p2, _, _ = plane_problem(14, 0.0, seed=41)
    r = hn.find_homography(p1[:3], p2[:3])
    assert r.count == 0 and r.iters == 0 and not r.mask.any() and not r.H.any()
    r = hn.find_homography(p1[:4], p2[:4])
    assert r.count == 4 and r.iters == 0 and r.mask.all() and r.H[2, 2] == 1
    assert np.abs(transfer(r.H, p1[:4]) - p2[:4]).max() <= 1e-9
    line = np.c_[np.linspace(10, 900, 40), np.linspace(20, 300, 40)].astype(np.float32)
    for a, b in ((line, line + 2), (np.full((30, 2), 7, np.float32), np.full((30, 2), 9, np.float32)),
                 (np.array([[0, 0], [5, 5], [10, 10], [3, 9]], np.float32),) * 2):
        r = hn.find_homography(a, b, max_iters=200)
        assert r.count == 0 and not r.mask.any() and not r.H.any()


def test_refit_and_polish_reproduce_the_true_h():
    p1, p2, R, t, normal, d = plane_scene(800, seed=3)
    Ht = hn.homography_from_pose(R, t, normal, d, K4)
    inl = np.ones(800, bool)
    inl[::7] = False
    start = Ht.reshape(9) * (1 + np.random.default_rng(4).normal(size=9) * 1e-3)
    H = hn.refit_polish(start / start[8], p1, p2, inl)
    corners = np.array([[0, 0], [W, 0], [W, H_IMG], [0, H_IMG]], np.float64)
    err = np.abs(transfer(H, corners) - transfer(Ht, corners)).max()
    print(f"refit + polish on noise-free data: corner transfer error {err:.3e} px")
    assert err <= 1e-8
    # the polish alone, from the perturbed start
    err = np.abs(transfer(hn.polish(start / start[8], p1, p2, inl), corners) - transfer(Ht, corners)).max()
    assert err <= 1e-8


def test_tree_sum_is_a_sum():
    rng = np.random.default_rng(8)
    for n in (1, 63, 256, 257, 1000):
        T = rng.normal(size=(n, 3))
        assert np.abs(hn.tree_sum(T) - T.sum(0)).max() <= 1e-12


# ---- the decomposition ----
def decomposition_cases():
    cases = []
    for normal in ((0, 0, 1.0), (0.1, -0.25, 1.0), (0.5, 0.1, 1.0), (-0.3, 0.6, 1.0)):
        nn = np.asarray(normal) / np.linalg.norm(normal)
        across = np.cross(nn, [0.3, 1.0, 0.2])
        for t in (nn * 0.7, -nn * 0.4, across / np.linalg.norm(across) * 0.8, [0.6, -0.1, 0.4]):
            cases.append((rot([0.02, -0.05, 0.015]), np.asarray(t, np.float64), nn, 8.0))
    return cases


def test_decomposition_against_its_definition():
    for R, t, normal, d in decomposition_cases():
        H = hn.homography_from_pose(R, t, normal, d, K4)
        Hn = hn.normalised_h(H, K4)
        sols = hn.decompose(H, K4)
        assert len(sols) == 4
        best = np.inf
        for k, (Rs, ts, ns) in enumerate(sols):
            M = Rs + np.outer(ts, ns)
            assert np.linalg.norm(Hn - M) / np.linalg.norm(Hn) <= 1e-12
            assert abs(np.linalg.det(Rs) - 1) <= 1e-12 and np.abs(Rs @ Rs.T - np.eye(3)).max() <= 1e-12
            assert abs(np.linalg.norm(ns) - 1) <= 1e-12
            best = min(best, max(np.abs(Rs - R).max(), np.abs(ts - t / d).max(), np.abs(ns - normal).max()))
        # t along the normal makes the two solutions meet: a double eigenvalue, whose square root loses half the digits
        assert best <= (1e-6 if abs(abs(t @ normal) - np.linalg.norm(t)) < 1e-12 else 1e-9), best
        # the order: pairs of opposite sign, the first of each with nz > 0, `a` the larger normal by (nz, ny, nx)
        for k in (0, 2):
            assert np.array_equal(sols[k][0], sols[k + 1][0]) and np.array_equal(sols[k][1], -sols[k + 1][1])
            assert np.array_equal(sols[k][2], -sols[k + 1][2]) and sols[k][2][2] > 0
        assert tuple(sols[0][2][::-1]) >= tuple(sols[2][2][::-1])


def test_decomposition_of_a_pure_rotation_and_of_a_singular_matrix():
    R = rot([0.03, -0.08, 0.02])
    sols = hn.decompose(hn.homography_from_pose(R, np.zeros(3), np.array([0, 0, 1.0]), 5.0, K4), K4)
    assert len(sols) == 1
    Rs, ts, ns = sols[0]
    assert np.abs(Rs - R).max() <= 1e-12 and not ts.any() and list(ns) == [0, 0, 1]
    assert abs(np.linalg.det(Rs) - 1) <= 1e-12
    assert hn.decompose(np.zeros(9), K4) == [] and hn.decompose(np.outer([1, 2, 3], [1, 1, 1.0]), K4) == []


# ---- the pose ----
def pose_fixture(normal, seed=5, n=400, t=(0.6, -0.1, 0.4)):
    p1, p2, R, t, normal, d = plane_scene(n, seed, normal=normal, t=t, R=rot([0.02, -0.05, 0.015]))
    return p1.astype(np.float32), p2.astype(np.float32), R, t, normal, d


def test_pose_picks_the_true_candidate_for_a_tilted_plane():
    p1, p2, R, t, normal, d = pose_fixture((0.5, 0.1, 1.0))
    H = hn.homography_from_pose(R, t, normal, d, K4)
    Rg, tg, ng, good4, mask = hn.homography_pose(H, p1, p2, K4)
    assert np.abs(Rg - R).max() <= 1e-9 and np.abs(tg - t / np.linalg.norm(t)).max() <= 1e-9 and np.abs(ng - normal).max() <= 1e-9
    assert good4[int(np.argmax(good4))] == len(p1) and sorted(good4)[-2] < len(p1) and mask.all()
    keep = (np.arange(len(p1)) % 3 != 0).astype(np.uint8)
    *_, good4m, maskm = hn.homography_pose(H, p1, p2, K4, mask=keep)
    assert np.array_equal(maskm, keep) and max(good4m) == keep.sum()


def test_fronto_parallel_plane_shows_the_two_way_tie():
    p1, p2, R, t, normal, d = pose_fixture((0.0, 0.0, 1.0), t=(0.1, 0.0, 0.5))      # head-on: the camera moves at the plane
    H = hn.homography_from_pose(R, t, normal, d, K4)
    Rg, tg, ng, good4, mask = hn.homography_pose(H, p1, p2, K4)
    top = sorted(good4)
    assert top[-1] == top[-2] == len(p1), good4          # both solutions put every point in front of both cameras
    assert good4[0] == len(p1)                            # and the first of them is the one picked
    sols = hn.decompose(H, K4)
    assert np.array_equal(Rg, sols[0][0]) and np.array_equal(ng, sols[0][2])
    assert min(np.abs(s[0] - R).max() + np.abs(s[2] - normal).max() for s in sols) <= 1e-9


# ---- the bound of the GPU equality test ----
def test_summation_order_sensitivity():
    worst, margins = 0.0, 0
    for n in SIZES:
        for outliers in OUTLIERS:
            for noise in NOISES:
                for seed in SEEDS:
                    p1, p2, r = equality_fixture(n, outliers, noise, seed)
                    assert r.margin_ok, ("fixture too close to the threshold for an equality test", n, outliers, noise, seed)
                    margins += 1
                    if r.count <= 4:
                        continue
                    inl = r.mask != 0
                    back = hn.refit_polish(r.H_loop, p1[::-1], p2[::-1], inl[::-1])
                    worst = max(worst, np.abs(unit_h(back) - unit_h(r.H)).max())
    print(f"summation-order sensitivity of the refit + polish over {margins} fixtures: d = {worst:.3e}")
    assert 0 < worst <= D_SENSITIVITY
