"""The restatement of the robust kernels (tests/pg_robust_numpy.py) against itself, and the conditions the fixtures of
tests/pg_robust_fixtures.py must meet on the arbiter before any GPU test rests on them.  CPU only."""
import numpy as np
import pytest

import pg_info_arbiter as arb
import pg_robust_fixtures as fx
import pg_robust_numpy as rn
from pg_info_fixtures import rms_translation

CS = np.concatenate([[0.0], 10.0 ** np.linspace(-8, 4, 97)])


@pytest.mark.parametrize("kind", [rn.HUBER, rn.CAUCHY, rn.GEMAN_MCCLURE])
@pytest.mark.parametrize("delta", [0.03, 0.7, 12.0])
def test_weight_is_the_derivative_of_rho(kind, delta):
    """Central differences with h = 1e-6 c, away from Huber's kink.  Their truncation error is h^2 rho''' / 6: with c rho''' / rho' of
    order 1 / c^2 ... 10 / c^2 for these three, 1e-11 relative -- 1e-9 allowed.  Their rounding error is the two roundings of rho
    over 2 h: eps rho / h, which is NOT small relative to w where rho has saturated (Geman-McClure far out: rho -> mu, w -> 0), so
    it is allowed as it is, four times over."""
    c = CS[1:]
    if kind == rn.HUBER:
        c = c[np.abs(c - delta * delta) > 1e-3 * delta * delta]
    h = 1e-6 * c
    fd = (rn.rho(kind, delta, c + h) - rn.rho(kind, delta, c - h)) / (2 * h)
    w = rn.weight(kind, delta, c)
    assert np.all(np.abs(fd - w) <= 1e-9 * w + 4 * np.finfo(float).eps * rn.rho(kind, delta, c) / h)
    near = c < 10 * (delta if kind == rn.GEMAN_MCCLURE else delta * delta)      # where that allowance is below 1e-8 w
    assert near.sum() > 20 and np.allclose(fd[near], w[near], rtol=1e-8, atol=0)


def test_dcs_is_the_table_not_the_derivative():
    phi = 0.5
    for c, s in ((0.1, None), (0.5, None), (1.5, 2 * 0.5 / 2.0), (50.0, 1.0 / 50.5)):
        w, r = float(rn.weight(rn.DCS, phi, c)), float(rn.rho(rn.DCS, phi, c))
        if s is None:
            assert (w, r) == (1.0, c)
        else:
            assert w == pytest.approx(s * s, rel=1e-15) and r == pytest.approx(s * s * c, rel=1e-15)
    c = 1.5
    fd = float(rn.rho(rn.DCS, phi, c + 1e-6) - rn.rho(rn.DCS, phi, c - 1e-6)) / 2e-6
    assert abs(fd - float(rn.weight(rn.DCS, phi, c))) > 0.1      # g2o's weight is not rho'


def test_continuity_at_the_branch_points():
    for delta in (0.03, 0.7, 12.0):
        b = delta * delta
        for f in (rn.rho, rn.weight):
            lo, hi = float(f(rn.HUBER, delta, b * (1 - 1e-13))), float(f(rn.HUBER, delta, b * (1 + 1e-13)))
            assert lo == pytest.approx(hi, rel=1e-12)
            lo, hi = float(f(rn.DCS, delta, delta * (1 - 1e-13))), float(f(rn.DCS, delta, delta * (1 + 1e-13)))
            assert lo == pytest.approx(hi, rel=1e-12)


@pytest.mark.parametrize("kind", rn.KINDS)
def test_weights_lie_in_0_1(kind):
    for delta in (1e-3, 0.7, 1e3):
        w = rn.weight(kind, delta, CS)
        assert np.all(w > 0) and np.all(w <= 1) and float(rn.weight(kind, delta, 0.0)) == 1.0
        assert np.all(np.diff(w) <= 0)                            # never growing with chi2
    assert np.all(rn.weight(rn.NONE, 1.0, CS) == 1) and np.array_equal(rn.rho(rn.NONE, 1.0, CS), CS)


def test_geman_mcclure_is_the_line_process():
    """Open3D's objective for an uncertain edge, mu (sqrt(l) - 1)^2 + l c, at its minimiser l = (mu / (mu + c))^2 equals rho."""
    for mu in (0.03, 2.0):
        l = rn.weight(rn.GEMAN_MCCLURE, mu, CS)
        assert np.allclose(mu * (np.sqrt(l) - 1) ** 2 + l * CS, rn.rho(rn.GEMAN_MCCLURE, mu, CS), rtol=1e-13, atol=1e-300)


@pytest.mark.parametrize("kind", rn.KINDS)
def test_an_irls_step_is_the_arbiters_step_with_scaled_information(kind):
    est, _, _, edges, _ = fx.graph("130f")
    om = fx.omegas("130f", "d")
    kern = fx.kernels_everywhere("130f", kind)
    X1 = rn.irls_step(est, edges, None, kern)[0]                   # one step, so that the odometry edges have residuals
    Xn, dx, info, (c, w, r) = rn.irls_step(X1, edges, om, kern)
    scaled = [float(rn.weight(kind, fx.KERNELS[kind], e6 @ om[k] @ e6)) * om[k]
              for k, (i, j, e6, A, B) in enumerate(arb.linearize(X1, edges))]
    Xa, dxa, _ = arb.step(X1, edges, scaled)
    assert np.array_equal(Xn, Xa) and np.array_equal(dx, dxa)
    assert np.any(w < 1) and np.all(w > 0)


# ---- the conditions on the fixtures ----------------------------------------------------------------------------------
@pytest.mark.parametrize("om_kind", ["i", "d"])
def test_condition_1_geman_mcclure_separates_the_false_closure(om_kind):
    _, _, _, edges, _ = fx.graph("130f")
    X = fx.gm_run("130f", om_kind)[-1]
    c, w, r = rn.edge_values(X, edges, fx.omegas("130f", om_kind), fx.kernels_on_closures("130f"))
    k_false = fx.false_edge_index()
    true = [k for k in fx.closure_indices("130f") if k != k_false]
    print(f"\nset {om_kind}: false closure w = {w[k_false]:.3e}, true closures w = {w[true]}")
    assert w[k_false] < fx.PRUNE_THRESHOLD and np.all(w[true] > 0.5)
    assert np.all(np.delete(w, fx.closure_indices("130f")) == 1)


@pytest.mark.parametrize("om_kind", ["i", "d"])
@pytest.mark.parametrize("name", fx.CASES)
def test_conditions_2_and_3_branch_points_and_conditioning(name, om_kind):
    """At the iterates the GPU tests check: four steps with each kind on every edge, and the ten Geman-McClure steps."""
    est, _, _, edges, _ = fx.graph(name)
    om = fx.omegas(name, om_kind)
    worst_cond, worst_margin = 0.0, np.inf
    for kind in rn.KINDS:
        kern = fx.kernels_everywhere(name, kind)
        X = est
        for it in range(4):
            Xn, dx, info, (c, w, r) = rn.irls_step(X, edges, om, kern)
            worst_margin = min(worst_margin, fx.branch_margin(kind, fx.KERNELS[kind], c))
            worst_cond = max(worst_cond, float(np.linalg.cond(info["H"].toarray())))
            X = Xn
    for X in fx.gm_run(name, om_kind)[:-1]:
        c, w, r = rn.edge_values(X, edges, om, fx.kernels_on_closures(name))
        H = arb.normal_equations(arb.linearize(X, edges), rn.weighted_omegas(om, w), len(X))[0]
        worst_cond = max(worst_cond, float(np.linalg.cond(H.toarray())))
    print(f"\n{name} / {om_kind}: largest cond(H) {worst_cond:.2e}, smallest branch-point margin {worst_margin:.2e}")
    assert worst_margin > 1e-6
    assert worst_cond <= 5.6e6


def test_condition_4_the_false_closure_does_the_damage_and_the_prune_undoes_it():
    est, _, _, edges, gt = fx.graph("130f")
    k_false = fx.false_edge_index()
    clean = fx.without_edge(edges, k_false)
    assert [(i, j) for i, j, _ in clean] == [(i, j) for i, j, _ in fx.graph("130")[3]]
    rms_bad = rms_translation(arb.optimize(est, edges, None, 10), gt)
    rms_clean = rms_translation(arb.optimize(est, clean, None, 10), gt)
    print(f"\nno kernel: rms translation {rms_clean:.4f} m without the false closure, {rms_bad:.4f} m with it")
    assert rms_bad >= 3 * rms_clean
    # with the kernel: optimise, prune (condition 1), optimise again -- against the graph that never had the edge
    kern_clean = fx.without_edge(fx.kernels_on_closures("130f"), k_false)
    X10 = fx.gm_run("130f", "i")[-1]
    rms_pruned = rms_translation(rn.irls(X10, clean, None, kern_clean, 10)[0], gt)
    rms_never = rms_translation(fx.gm_run("130", "i")[-1], gt)
    print(f"Geman-McClure: {rms_pruned:.4f} m after the prune, {rms_never:.4f} m on the graph that never had the edge")
    assert rms_pruned <= 1.1 * rms_never
