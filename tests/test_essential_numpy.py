"""The essential-matrix restatement (tests/essential_numpy.py) against geometry it must reproduce: the true E among the
five-point solutions, both constraints on every solution, the polynomial coefficient matrix against a direct
evaluation, and recoverPose's choice of the true (R, t)."""
import numpy as np

import essential_numpy as en


def rot(a):
    a = np.asarray(a, np.float64)
    th = np.linalg.norm(a)
    k = a / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def five_point_samples(count, seed=0):
    """noise-free 5-samples of random two-view geometries: normalised q1, q2 and the true E."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        R = rot(rng.normal(size=3) * 0.3)
        t = rng.normal(size=3)
        t /= np.linalg.norm(t)
        X = np.c_[rng.uniform(-2, 2, (5, 2)), rng.uniform(3, 8, 5)]
        X2 = X @ R.T + t
        out.append((X[:, :2] / X[:, 2:], X2[:, :2] / X2[:, 2:], en.essential_from_pose(R, t)))
    return out


def test_five_point_finds_the_true_essential_matrix():
    for q1, q2, E in five_point_samples(500):
        S = en.five_point(q1, q2)
        assert 1 <= len(S) <= 10
        assert min(np.abs(s - E).max() for s in S) <= 1e-9
        for s in S:
            assert abs(np.linalg.norm(s) - 1) < 1e-12
            det, trace = en.constraint_residuals(s)
            assert det <= 1e-10 and trace <= 1e-10
            h1, h2 = np.c_[q1, np.ones(5)], np.c_[q2, np.ones(5)]
            assert np.abs(np.einsum("ij,jk,ik->i", h2, s, h1)).max() < 1e-10  # x2^T E x1 = 0 on the sample


def test_coefficient_matrix_evaluates_the_constraints():
    """row r of the 10 x 20 matrix times the monomial vector = constraint r of E(x, y, z), at random (x, y, z)."""
    rng = np.random.default_rng(1)
    q1, q2, _ = five_point_samples(1, seed=5)[0]
    basis = en.null_basis(q1, q2)
    A = en.coeff_matrix(basis)
    for _ in range(20):
        x, y, z = rng.normal(size=3)
        m = np.array([x ** a * y ** b * z ** c for a, b, c in en.MONO])
        E = (basis[0] * x + basis[1] * y + basis[2] * z + basis[3]).reshape(3, 3)
        EEt = E @ E.T
        want = np.concatenate([(2 * EEt @ E - np.trace(EEt) * E).ravel(), [np.linalg.det(E)]])
        assert np.allclose(A @ m, want, rtol=1e-12, atol=1e-12)


def test_sampson_error_is_float():
    q1, q2, E = five_point_samples(1, seed=2)[0]
    e = en.sampson(E, q1, q2)
    assert e.dtype == np.float32 and float(e.max()) < 1e-20


def scene(n, seed, R, t, K4=(718.856, 718.856, 607.1928, 185.2157)):
    rng = np.random.default_rng(seed)
    X = np.c_[rng.uniform(-15, 15, n), rng.uniform(-4, 1.5, n), rng.uniform(4, 35, n)]
    X2 = X @ R.T + t

    def px(P):
        return np.c_[K4[0] * P[:, 0] / P[:, 2] + K4[2], K4[1] * P[:, 1] / P[:, 2] + K4[3]]

    return px(X), px(X2), X


def test_recover_pose_picks_the_true_pose():
    K4 = (718.856, 718.856, 607.1928, 185.2157)
    for seed in range(5):
        rng = np.random.default_rng(100 + seed)
        R = rot(rng.normal(size=3) * 0.05)
        t = np.array([0.1, -0.05, 1.0]) + rng.normal(size=3) * 0.1
        p1, p2, _ = scene(300, seed, R, t, K4)
        E = en.essential_from_pose(R, t)
        Rr, tr, good, mask, g = en.recover_pose(E, p1, p2, K4)
        assert np.abs(Rr - R).max() < 1e-6
        assert np.abs(tr - t / np.linalg.norm(t)).max() < 1e-6
        assert good == 300 and mask.all() and sorted(g)[-2] < good


def test_ransac_restatement_finds_the_inliers(orc):
    K4 = (718.856, 718.856, 607.1928, 185.2157)
    R, t = rot([0.01, 0.04, -0.02]), np.array([0.1, -0.05, 1.0])
    p1, p2, _ = scene(200, 7, R, t, K4)
    p2 = en.push_off_epipolar(p1, p2, K4, R, t, np.random.default_rng(8).uniform(8, 30, 60), np.arange(60))
    E, mask, count, iters = en.find_essential(p1.astype(np.float32), p2.astype(np.float32), K4, seed=3)
    assert count == 140 and mask[60:].all() and not mask[:60].any()
    assert 0 < iters < 1000
    assert np.abs(E[0] - en.essential_from_pose(R, t)).max() < 1e-5
