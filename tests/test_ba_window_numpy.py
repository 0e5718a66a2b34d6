"""The float64 restatement of svo_ba_window (tests/ba_window_numpy.py) held to (1) a dense Levenberg-Marquardt over every unknown with
numeric Jacobians (tests/ba_window_fixtures.py), (2) the standing oracle of BundleAdjust3d2d at one pose, and (3) itself; and the proof
that the fixtures reach the branches they are named for.  CPU only.  The tolerances are the ones tests/test_oracle_ba.py sets
between a Schur form and a dense solver.  Largest deviations measured over the cases below: t 1.4e-11, R 7.2e-13, X 3.6e-10."""
import numpy as np
import pytest

import ba_window_fixtures as F
import ba_window_numpy as M
from ba_fixtures import K4 as K4_ONE, problem


@pytest.fixture(scope="module")
def solved():
    """Every named case through the restatement once, with its trial trace."""
    out = {}
    for name in F.CASES:
        w, p = F.case(name)
        trace = []
        out[name] = (w, p, M.ba_window(*F.args(w), p, trace=trace), trace)
    return out


@pytest.mark.parametrize("name", list(F.CASES))
def test_schur_form_follows_the_dense_lm(solved, name):
    w, p, (P, X, chi, info), _ = solved[name]
    Pd, Xd, infod = F.dense_lm(*F.args(w), p)
    dev = F.check_close(P, X, info, Pd, Xd, infod, pytest.approx)
    print(name, dev)


def test_cases_cover_what_the_issue_names():
    shapes = {(wk["n"], wk["n_poses"]) for wk, _ in F.CASES.values()}
    assert {(12, 2), (40, 4)} <= shapes and {n for n, _ in shapes} == {12, 40} and {q for _, q in shapes} == {2, 4}
    assert any(not wk.get("fixed", (0,)) for wk, _ in F.CASES.values()) and any(wk.get("fixed", (0,)) for wk, _ in F.CASES.values())
    assert any(pk.get("huber_mono", 0) > 0 for _, pk in F.CASES.values()) and any(not pk.get("huber_mono", 0) for _, pk in F.CASES.values())
    assert {wk.get("obs", "mixed") for wk, _ in F.CASES.values()} == {"mono", "stereo", "mixed"}


def test_fixtures_reach_their_branches(solved):
    # a rejected trial, followed by an accepted one
    _, _, (_, _, _, info), trace = solved["n40_p2_rejects"]
    assert [a for a, _ in trace].count(False) >= 1 and trace[-1][0] and info["trials"] > info["iterations"]
    # Huber: active on some observations, inactive on others, at the start and at the end
    w, p, (P, X, chi, _), _ = solved["n40_p4_mixed_fixed_huber"]
    op = M.csr_points(w["obs_start"])
    e, stereo, _ = M.residuals(w["poses"], w["pts3d"].astype(np.float64), op, w["obs_pose"], w["obs_uvr"], p)
    delta = np.where(stereo, p["huber_stereo"], p["huber_mono"])
    for e2 in ((e * e).sum(1), chi):
        assert (e2 > delta ** 2).any() and (e2 <= delta ** 2).any()
    assert (stereo & (chi > delta ** 2)).any() or (~stereo & (chi > delta ** 2)).any()
    # points seen by one pose only, by two, by all; a held pose with observations
    for name in ("n40_p4_mixed_fixed", "n12_p2_mixed_fixed"):
        w = solved[name][0]
        runs = np.diff(w["obs_start"])
        assert (runs == 1).any() and (runs == len(w["fixed"])).any() and (len(w["fixed"]) == 2 or (runs == 2).any())
        assert w["fixed"][0] == 1 and (w["obs_pose"] == 0).sum() >= 3
    w = solved["n40_p4_mixed_fixed"][0]
    assert np.isnan(w["obs_uvr"][:, 2]).any() and (~np.isnan(w["obs_uvr"][:, 2])).any()


@pytest.mark.parametrize("name", F.ANCHORED)
def test_chi2_does_not_collapse_and_the_poses_improve(solved, name):
    w, p, (P, X, chi, info), _ = solved[name]
    assert info["chi2_after"] < info["chi2_before"] and info["chi2_after"] > 1e-3 * info["chi2_before"]
    free = np.flatnonzero(w["fixed"] == 0)
    e0 = np.linalg.norm(w["poses"][free, 9:] - w["truth"][free, 9:], axis=1)
    e1 = np.linalg.norm(P[free, 9:] - w["truth"][free, 9:], axis=1)
    assert (e1 < 0.5 * e0).all(), (e0, e1)
    assert np.array_equal(P[w["fixed"] == 1], w["poses"][w["fixed"] == 1])


@pytest.mark.parametrize("n", [5, 440])
def test_one_pose_is_the_standing_oracle(orc, n):
    uv, X, R0, t0, _ = problem(n, 3 if n == 440 else 1, noise=0.2)
    p = M.params(fx=K4_ONE[0], fy=K4_ONE[0], cx=K4_ONE[2], cy=K4_ONE[3], iterations=6)
    uvr = np.c_[uv, np.full(n, np.nan, np.float32)].astype(np.float32)
    P, Xw, chi, info = M.ba_window(np.r_[R0.ravel(), t0][None], [0], X, np.arange(n + 1), np.zeros(n, np.int32), uvr, p)
    t, R, Xo, io = orc.ba_3d2d(uv, X, K4_ONE, R0, t0, iterations=6)
    io = dict(io)
    F.check_close(P, Xw, info, np.r_[R.ravel(), t][None], Xo, io, pytest.approx)


def test_huber_weight_is_the_derivative_of_rho():
    delta = 2.5
    for e2 in (0.3, 6.0, 6.5, 40.0, 900.0):
        h = 1e-6 * e2
        (rp, _), (rm, _) = M.huber(e2 + h, delta), M.huber(e2 - h, delta)
        rho, w = M.huber(e2, delta)
        assert float(w) == pytest.approx((float(rp) - float(rm)) / (2 * h), rel=1e-6)
        assert float(rho) == (e2 if e2 <= delta * delta else 2 * np.sqrt(e2) * delta - delta * delta)
    assert M.huber(6.25, delta) == (6.25, 1.0)              # e2 == delta^2: still quadratic
    assert M.huber(123.0, 0.0) == (123.0, 1.0)              # delta 0: no kernel


def test_zero_deltas_give_the_bits_of_no_kernel(solved):
    w, p, (P, X, chi, info), _ = solved["n40_p4_mixed_fixed"]
    assert p["huber_mono"] == 0 and p["huber_stereo"] == 0
    P2, X2, chi2, info2 = M.ba_window(*F.args(w), p, no_kernel=True)
    assert np.array_equal(P, P2) and np.array_equal(X, X2) and np.array_equal(chi, chi2) and info == info2


def test_unobserved_points_come_back_untouched_and_zero_iterations_move_nothing():
    w = F.window(n=40, n_poses=3, seed=9, unobserved=(0, 17, 39))
    p = F.prm(iterations=4)
    P, X, chi, info = M.ba_window(*F.args(w), p)
    for i in (0, 17, 39):
        assert np.array_equal(X[i], w["pts3d"][i].astype(np.float64))
    assert len(chi) == info["observations"] == w["obs_start"][-1] and info["chi2_after"] < info["chi2_before"]
    P0, X0, chi0, info0 = M.ba_window(*F.args(w), F.prm(iterations=0))
    assert np.array_equal(P0, w["poses"]) and np.array_equal(X0, w["pts3d"].astype(np.float64))
    assert info0["iterations"] == 0 and info0["trials"] == 0 and info0["chi2_before"] == info0["chi2_after"] == pytest.approx(chi0.sum())
