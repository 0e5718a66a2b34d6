"""The ICP restatement (tests/icp_numpy.py) against independent arithmetic, on the CPU: its normals against
numpy.linalg.eigh, its information matrix against an einsum of the rows of G, its ICP against the pose the corner source
was moved by, the branches its fixtures are named for, and the conversion of Lambda to an edge's information
(svo_icp_edge_information, host code of the library) against finite differences of the graph's own error."""
import numpy as np
import pytest
from scipy.spatial.transform import Rotation as Rot

import icp_fixtures as fx
import icp_numpy as ref
from ros_stereo_slam_amd import capi

EIG_CASES = ["corner_pair", "corner_4097", "n_tgt_65"]


@pytest.mark.parametrize("name", EIG_CASES)
def test_normals_against_eigh(name):
    """First-order bound on the eigenvector: 2^-52 lambda_max / gap ~ 2e-13 rad at gap >= 1e-3 lambda_max; asserted at
    1e-9 rad, four decades above, which covers the Jacobi solver's own rounding."""
    r = fx.reference(name)
    w, v = np.linalg.eigh(r["cov"])
    assert np.all(r["cnt"] >= 3)
    gap = (w[:, 1] - w[:, 0]) / w[:, 2]
    assert gap.min() >= 1e-3, f"fixture {name}: eigenvalue gap {gap.min():.2e} of lambda_max"
    n = r["normals"]
    assert np.abs(np.linalg.norm(n, axis=1) - 1).max() < 1e-15
    c = np.abs(np.sum(n * v[:, :, 0], axis=1))
    s = np.linalg.norm(np.cross(n, v[:, :, 0]), axis=1)
    ang = np.arctan2(s, c)
    print(f"{name}: worst angle to eigh {ang.max():.2e} rad, smallest gap {gap.min():.2e}")
    assert ang.max() <= 1e-9


def test_degenerate_normals():
    for name in ("n_tgt_1", "n_tgt_2"):
        assert np.array_equal(fx.reference(name)["normals"], np.tile([0.0, 0.0, 1.0], (len(fx.cases()[name]["tgt"]), 1)))
    n = fx.reference("plane")["normals"]
    assert np.array_equal(np.abs(n), np.tile([0.0, 0.0, 1.0], (len(n), 1)))  # an exact plane: exact zeros stay zeros
    n = fx.reference("collinear")["normals"]
    d = np.array([1.0, 2.0, -1.0]) / np.sqrt(6.0)
    assert np.all(np.isfinite(n)) and np.abs(n @ d).max() < 1e-6  # rank one: some unit vector across the line
    assert np.abs(np.linalg.norm(n, axis=1) - 1).max() < 1e-15


@pytest.mark.parametrize("name", sorted(fx.cases()))
def test_information_against_einsum(name):
    r, c = fx.reference(name), fx.cases()[name]
    E = ref.information_einsum(c["tgt"], r["info_corr"])
    n = max(r["n_corr"], 1)
    scale = max(np.abs(E).max(), 1.0)
    assert np.abs(r["info"] - E).max() <= n * 2.0 ** -52 * scale
    assert np.array_equal(r["info"], r["info"].T)


def test_icp_recovers_known_pose():
    """The source was rounded to float32 at about 12 m: 2^-21 m ~ 5e-7 m per coordinate.  Ten times that: 1e-5 m and, at
    that lever arm, 1e-6 rad."""
    T = fx.reference("corner_pair")["pair"][0]
    K = fx.known_pose()
    D = T @ np.linalg.inv(K)
    # the rotation about the cloud, not about the origin: compare where the cloud's centre lands
    c = np.r_[fx.cases()["corner_pair"]["tgt"].astype(np.float64).mean(0), 1.0]
    dt = np.linalg.norm((D @ c - c)[:3])
    dr = np.linalg.norm(Rot.from_matrix(D[:3, :3]).as_rotvec())
    print(f"corner pair: translation error at the cloud's centre {dt:.2e} m, rotation error {dr:.2e} rad")
    assert dt <= 1e-5 and dr <= 1e-6


def test_fixtures_reach_their_branches():
    R = {k: fx.reference(k) for k in fx.cases()}
    assert R["duplicates"]["rec"]["ties"] >= 60 and np.all(R["duplicates"]["corr"][:60] < 20)
    assert R["duplicates"]["rec"]["no_corr"] == 0
    assert R["far"]["rec"]["no_corr"] > 0 and np.all(R["far"]["corr"] == -1) and R["far"]["fitness"] == 0.0
    assert R["far"]["rec"]["identity_update"] == 1 and R["far"]["icp"][3] == 1
    assert np.array_equal(R["far"]["icp"][0], np.eye(4))
    assert R["plane"]["n_corr_step"] > 0 and R["plane"]["rec"]["identity_update"] >= 1
    assert np.array_equal(R["plane"]["icp"][0], np.eye(4)) and R["plane"]["icp"][3] == 1
    its = R["corner_pair"]["pair"][2][3], R["corner_pair"]["pair"][3][3]
    assert 1 < its[0] < 30 and 1 <= its[1] < 30, its
    assert R["corner_pair"]["rec"]["identity_update"] == 0
    assert len(R["n_tgt_2"]["knn"][0]) == 3 and np.array_equal(R["n_tgt_2"]["knn"], [[0, 1, -1], [1, 0, -1]])
    assert len(fx.cases()["corner_4097"]["tgt"]) == 64 * 64 + 1
    assert {len(c["tgt"]) for c in fx.cases().values()} >= {1, 2, 63, 64, 65, 4097}
    assert {len(c["src"]) for c in fx.cases().values()} >= {1, 65, 300}


def _graph_error(Z, X):
    """e = [t ; s q_xyz] of Z^-1 X, s making q_w >= 0"""
    E = np.linalg.inv(Z) @ X
    q = Rot.from_matrix(E[:3, :3]).as_quat()
    if q[3] < 0:
        q = -q
    return np.r_[E[:3, 3], q[:3]]


def _exp_se3(xi):
    """exp of [w ; v] as a 4 x 4 matrix (series)"""
    A = np.zeros((4, 4))
    A[:3, :3] = ref.skew(xi[:3])
    A[:3, 3] = xi[3:]
    out, term = np.eye(4), np.eye(4)
    for k in range(1, 12):
        term = term @ A / k
        out = out + term
    return out


def test_edge_information_rule():
    """Perturb T by +-1e-6 along each axis on the left: e^T Omega e must equal xi^T Lambda xi to 1e-5 relative (the
    central difference is O(h^2); e's second-order term is O(h) relative)."""
    r = fx.reference("corner_pair")
    T, L = r["pair"][0], r["pair"][1]
    Om = capi.info_matrix(capi.icp_edge_information(L, T))
    assert np.allclose(Om, ref.edge_information(L, T), rtol=1e-12, atol=1e-12 * np.abs(Om).max())
    h = 1e-6
    rng = np.random.default_rng(0)
    dirs = list(np.eye(6)) + [rng.normal(size=6) for _ in range(4)]
    for d in dirs:
        xi = h * d / np.linalg.norm(d)
        e = 0.5 * (_graph_error(T, _exp_se3(xi) @ T) - _graph_error(T, _exp_se3(-xi) @ T))
        a, b = e @ Om @ e, xi @ L @ xi
        assert abs(a - b) <= 1e-5 * b, (d, a, b)


def test_edge_information_scales_exactly():
    r = fx.reference("corner_pair")
    T, L = r["pair"][0], r["pair"][1]
    assert np.array_equal(capi.icp_edge_information(4.0 * L, T), 4.0 * capi.icp_edge_information(L, T))


def test_meas7_matches_scipy():
    T = fx.known_pose()
    m = capi.icp_meas7(T)
    q = Rot.from_matrix(T[:3, :3]).as_quat()
    assert np.allclose(m[:3], T[:3, 3]) and np.allclose(m[3:], q if q[3] >= 0 else -q, atol=1e-15)
