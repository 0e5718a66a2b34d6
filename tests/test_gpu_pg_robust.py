"""Robust kernels on pose-graph edges and pruning (svo_pg_set_robust_kernel, svo_pg_set_loop_closure_kernel, svo_pg_edge_residuals,
svo_pg_prune_edges) on the GPU, against the blind restatement tests/pg_robust_numpy.py on the weighted arbiter
(tests/pg_info_arbiter.py).  The graphs and every parameter are those of tests/pg_robust_fixtures.py, whose conditions
tests/test_pg_robust_numpy.py asserts on the CPU.

The graph has no call that sets its estimates, so "at the arbiter's iterates" is taken as everywhere in test_gpu_posegraph_info.py:
iterations one at a time, the arbiter stepping from the graph's own estimates (which the same tests hold within 1e-8 of the
arbiter's)."""
import pathlib
import subprocess

import numpy as np
import pytest

import icp_fixtures as ifx
import pg_info_arbiter as arb
import pg_robust_fixtures as fx
import pg_robust_numpy as rn
from pg_info_fixtures import _inv7, _mul7, chain, rms_translation
from ros_stereo_slam_amd import capi, registration

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parents[1]
EPS_E = 1e-15   # rounding of an edge's error e: a few eps of poses within a metre (Z^-1 Xi^-1 Xj: three compositions)


def _build(ctx, name, om_kind="i", kernels=None, lc_kernel=None):
    """the chain node by node; lc_kernel = (kind, delta) is set before the first node, kernels (one per edge or None) after the last"""
    est, closures, el, edges, _ = fx.graph(name)
    g = capi.PoseGraph(ctx)
    if lc_kernel is not None:
        g.set_loop_closure_kernel(*lc_kernel)
    for i in range(1, len(est)):
        g.augment_node(est[i])
        for at, to in closures:
            if at == i:
                g.add_loop_closure(to)
    om = fx.omegas(name, om_kind)
    if om is not None:
        for e, Om in enumerate(om):
            g.set_edge_information(e, Om)
    for e, kd in enumerate(kernels or []):
        if kd is not None:
            g.set_robust_kernel(e, *kd)
    assert [(i, j) for i, j, _ in g.edges()] == [(i, j) for i, j, _ in edges]
    return g


def _lam_max(om_kind):
    return 1.0 if om_kind == "i" else 100.0


@pytest.mark.parametrize("kind", rn.KINDS)
@pytest.mark.parametrize("om_kind", ["i", "d"])
@pytest.mark.parametrize("name", ["40", "130"])
def test_unit_weights_change_no_bit(ctx, name, om_kind, kind):
    """A parameter so large that w == 1.0 on every edge (Huber: c <= d^2; Cauchy: 1 + c / d^2 rounds to 1; DCS: s >= 1;
    Geman-McClure: mu + c rounds to mu): the robust instantiation stores value * 1.0 -- the estimates and chi2[] of the graph
    without kernels, bit for bit, with and without information matrices."""
    n_e = len(fx.graph(name)[2])
    a = _build(ctx, name, om_kind)
    b = _build(ctx, name, om_kind, kernels=[(kind, 1e30)] * n_e)
    assert b.robust_kernel(n_e - 1) == (kind, 1e30) and a.robust_kernel(0) == (capi.PG_ROBUST_NONE, 0.0)
    for k in range(4):
        ca, cb = a.optimize(1), b.optimize(1)
        assert np.array_equal(ca, cb), k
        assert np.array_equal(a.estimates(), b.estimates()), k
        assert np.all(b.linearization_weights() == 1.0)
    with pytest.raises(capi.SvoError) as ei:
        a.linearization_weights()                                  # no kernel: the non-robust kernels ran, nothing was stored
    assert ei.value.code == capi.SVO_ERR_STATE
    a.close()
    b.close()


@pytest.mark.parametrize("kind", rn.KINDS)
@pytest.mark.parametrize("om_kind", ["i", "d"])
@pytest.mark.parametrize("name", fx.CASES)
def test_edge_residuals_against_the_restatement(ctx, name, om_kind, kind):
    """chi2, w and rho per edge along four iterations.  The graph's chi2 (their sum) to 1e-12 relative, the bound of
    test_gpu_posegraph_info.  Per edge the same 1e-12 (w, rho: 1e-11 -- their condition number in chi2 is <= 2, plus a decade) on
    top of what the rounding of e itself leaves: the odometry edges start at e = 0 exactly, where chi2 is 1e-31 of rounding and
    has no relative accuracy; d(chi2) = 2 |Om e| de + |Om| de^2 with de = EPS_E, |Om e| <= sqrt(lam_max chi2)."""
    _, _, _, edges, _ = fx.graph(name)
    om, kern = fx.omegas(name, om_kind), fx.kernels_everywhere(name, kind)
    g = _build(ctx, name, om_kind, kernels=kern)
    lam = _lam_max(om_kind)
    worst = np.zeros(4)
    for it in range(4):
        X = g.estimates()
        c, w, r = g.edge_residuals()
        cn, wn, rnn = rn.edge_values(X, edges, om, kern)
        floor = 2 * EPS_E * np.sqrt(lam * cn) + lam * EPS_E ** 2
        worst = np.maximum(worst, [abs(c.sum() - cn.sum()) / cn.sum(), np.max((np.abs(c - cn) - floor) / cn.clip(1e-300)),
                                   np.max(np.abs(w - wn) / wn), np.max((np.abs(r - rnn) - floor) / rnn.clip(1e-300))])
        assert abs(c.sum() - cn.sum()) <= 1e-12 * cn.sum()
        assert np.all(np.abs(c - cn) <= 1e-12 * cn + floor)
        assert np.all(np.abs(w - wn) <= 1e-11 * wn)
        assert np.all(np.abs(r - rnn) <= 1e-11 * rnn + floor)
        chi2 = g.optimize(1)
        assert chi2[0] == pytest.approx(c.sum(), rel=1e-13)         # chi2[] stays the unweighted sum
        c1, w1, _ = g.edge_residuals()
        assert np.array_equal(g.linearization_weights(), w1)        # slot 121 of the records of the final linearisation
        assert chi2[1] == pytest.approx(c1.sum(), rel=1e-13)
    print(f"\n{name} / {om_kind} / {rn.NAMES[kind]}: worst relative differences: sum chi2 {worst[0]:.1e}, chi2 {worst[1]:.1e} "
          f"(beyond the floor), w {worst[2]:.1e}, rho {worst[3]:.1e} (beyond the floor)")
    only = g.ctx.lib.svo_pg_edge_residuals(g._h, None, None, None)  # every output may be NULL
    assert only == capi.SVO_OK
    g.close()


@pytest.mark.parametrize("kind", rn.KINDS)
@pytest.mark.parametrize("om_kind", ["i", "d"])
@pytest.mark.parametrize("name", fx.CASES)
def test_irls_iterations_against_the_arbiter(ctx, name, om_kind, kind):
    """Four re-weighted iterations one at a time, kernels on every edge.  With one refinement pass: 1e-8.  The single solve: never
    further from the arbiter than 1.5 times one plain float64 Cholesky of the arbiter's own re-weighted system, or 1e-9.
    DESIGN.md section 10l has the measured deviations."""
    _, _, _, edges, _ = fx.graph(name)
    om, kern = fx.omegas(name, om_kind), fx.kernels_everywhere(name, kind)
    g = _build(ctx, name, om_kind, kernels=kern)
    r = _build(ctx, name, om_kind, kernels=kern)
    r.set_refinement(1)
    dev_g, dev_c, dev_r, acted = [], [], [], 0
    for k in range(4):
        X0 = g.estimates()
        g.optimize(1)
        Xa, dx, info, (c, w, _) = rn.irls_step(X0, edges, om, kern)
        assert fx.branch_margin(kind, fx.KERNELS[kind], c) > 1e-6    # (a condition of the fixture, at the GPU's own iterate)
        acted += int((w < 1).sum())
        dev_g.append(max(arb.deviation(g.estimates(), Xa)))
        dev_c.append(max(arb.deviation(arb.plain_cholesky_step(X0, info), Xa)))
        X0 = r.estimates()
        r.optimize(1)
        Xa = rn.irls_step(X0, edges, om, kern)[0]
        dev_r.append(max(arb.deviation(r.estimates(), Xa)))
    print(f"\n{name} / {om_kind} / {rn.NAMES[kind]} ({acted} weights below 1): GPU single solve {max(dev_g):.1e}, numpy Cholesky "
          f"{max(dev_c):.1e}, GPU refined {max(dev_r):.1e}")
    g.close()
    r.close()
    assert max(dev_r) <= 1e-8, dev_r
    assert max(dev_g) <= 1.5 * max(dev_c) or max(dev_g) <= 1e-9, (dev_g, dev_c)


@pytest.mark.parametrize("om_kind", ["i", "d"])
def test_false_closure_end_to_end(ctx, om_kind):
    est, _, el, edges, gt = fx.graph("130f")
    om = fx.omegas("130f", om_kind)
    k_false = fx.false_edge_index()
    g = _build(ctx, "130f", om_kind, lc_kernel=(capi.PG_ROBUST_GEMAN_MCCLURE, fx.MU))
    n_e = g.num_edges
    assert [g.robust_kernel(e)[0] for e in range(n_e)] == [capi.PG_ROBUST_GEMAN_MCCLURE if c else 0 for (_, _, c) in el]
    g.optimize(10)
    dev10 = max(arb.deviation(g.estimates(), fx.gm_run("130f", om_kind)[-1]))
    info_before = [g.edge_information(e) for e in range(n_e)]
    kern_before = [g.robust_kernel(e) for e in range(n_e)]
    edges_before = g.edges()
    w = g.edge_residuals()[1]
    assert w[k_false] < fx.PRUNE_THRESHOLD
    removed = g.prune_edges(fx.PRUNE_THRESHOLD)
    assert removed.tolist() == [k_false] and g.num_edges == n_e - 1
    for (i, j, z), (i2, j2, z2) in zip(g.edges(), fx.without_edge(edges_before, k_false)):
        assert (i, j) == (i2, j2) and np.array_equal(z, z2)
    for e in range(k_false, n_e - 1):                              # what moved: the later edges' information and kernels
        assert np.array_equal(g.edge_information(e), info_before[e + 1]) and g.robust_kernel(e) == kern_before[e + 1]
    assert g.prune_edges(fx.PRUNE_THRESHOLD).size == 0             # nothing else is below the threshold
    clean = fx.without_edge(edges, k_false)
    om_clean = None if om is None else fx.without_edge(om, k_false)
    kern_clean = fx.without_edge(fx.kernels_on_closures("130f"), k_false)
    X1 = g.estimates()
    g.optimize(10)
    Xa = rn.irls(X1, clean, om_clean, kern_clean, 10)[0]
    dev = max(arb.deviation(g.estimates(), Xa))
    rms, rms_never = rms_translation(g.estimates(), gt), rms_translation(fx.gm_run("130", om_kind)[-1], gt)
    print(f"\nset {om_kind}: ten iterations with the false closure {dev10:.1e} from the arbiter's; after the prune {dev:.1e}; "
          f"rms translation {rms:.4f} m, {rms_never:.4f} m on the graph that never had the edge")
    g.close()
    assert dev <= 1e-8
    assert rms <= 1.1 * rms_never


def test_loop_closure_kernel_applies_to_later_closures_only(ctx):
    est = fx.graph("40")[0]
    g = capi.PoseGraph(ctx)
    for p in est[1:6]:
        g.augment_node(p)
    g.add_loop_closure(0)                                            # edge 5: before the call
    g.set_loop_closure_kernel(capi.PG_ROBUST_CAUCHY, 0.7)
    assert g.robust_kernel(5) == (capi.PG_ROBUST_NONE, 0.0)
    g.augment_node(est[6])                                           # 6: odometry never gets one
    g.add_loop_closure(1)                                            # 7
    g.add_loop_closure(2, meas7=[0, 0, 0, 0, 0, 0, 1.0], info21=2 * np.eye(6))   # 8
    g.augment_nodes(est[7:10], closure_from=[3, -1, 4])              # 9 closure, 10, 11, 12 closure, 13
    g.set_loop_closure_kernel(capi.PG_ROBUST_NONE)
    g.add_loop_closure(0)                                            # 14
    kinds = [g.robust_kernel(e) for e in range(g.num_edges)]
    cauchy = (capi.PG_ROBUST_CAUCHY, 0.7)
    none = (capi.PG_ROBUST_NONE, 0.0)
    assert kinds == [none] * 7 + [cauchy, cauchy, cauchy, none, none, cauchy, none, none]
    assert np.all(np.isfinite(g.optimize(2)))
    g.close()


def test_refusals(ctx, tmp_path):
    g = _build(ctx, "40")
    n_e, GM = g.num_edges, capi.PG_ROBUST_GEMAN_MCCLURE
    for args in ((0, 5, 1.0), (0, -1, 1.0), (0, GM, 0.0), (0, GM, -1.0), (0, GM, float("nan")), (0, GM, float("inf")),
                 (n_e, GM, 1.0), (-1, GM, 1.0)):
        with pytest.raises(capi.SvoError) as ei:
            g.set_robust_kernel(*args)
        assert ei.value.code == capi.SVO_ERR_ARG, args
    for args in ((7, 1.0), (GM, 0.0), (GM, float("nan"))):
        with pytest.raises(capi.SvoError) as ei:
            g.set_loop_closure_kernel(*args)
        assert ei.value.code == capi.SVO_ERR_ARG, args
    with pytest.raises(capi.SvoError):
        g.robust_kernel(n_e)
    assert all(g.robust_kernel(e) == (0, 0.0) for e in range(n_e))
    assert g.prune_edges(0.25).size == 0                             # no kernel anywhere: nothing goes
    # capacity: the closure is below the threshold, no slot is offered -- nothing is removed
    g.set_robust_kernel(n_e - 1, GM, 1e-9)
    with pytest.raises(capi.SvoError) as ei:
        g.prune_edges(0.25, cap=0)
    assert ei.value.code == capi.SVO_ERR_CAPACITY and g.num_edges == n_e
    with pytest.raises(capi.SvoError) as ei:
        g.prune_edges(float("nan"))
    assert ei.value.code == capi.SVO_ERR_ARG and g.num_edges == n_e
    # an odometry edge with a kernel and a tiny weight stays (consecutive vertices), the closure goes
    g.optimize(1)
    g.set_robust_kernel(3, GM, 1e-300)
    assert g.edge_residuals()[1][3] < 0.25
    assert g.prune_edges(0.25).tolist() == [n_e - 1] and g.num_edges == n_e - 1
    g.close()
    # the disconnecting prune: vertex 2 hangs on a non-consecutive edge alone
    path = tmp_path / "tree.g2o"
    path.write_text("VERTEX_SE3:QUAT 0 0 0 0 0 0 0 1\nVERTEX_SE3:QUAT 1 1 0 0 0 0 0 1\nVERTEX_SE3:QUAT 2 2 0 0 0 0 0 1\n"
                    "EDGE_SE3:QUAT 0 1 1 0 0 0 0 0 1\nEDGE_SE3:QUAT 0 2 1.5 0 0 0 0 0 1\n")
    h = capi.PoseGraph(ctx)
    h.read_g2o(path)
    h.set_robust_kernel(1, GM, 1e-3)
    with pytest.raises(capi.SvoError) as ei:
        h.prune_edges(0.25)
    assert ei.value.code == capi.SVO_ERR_STATE and "vertex 2" in str(ei.value) and h.num_edges == 2
    assert h.robust_kernel(1) == (GM, 1e-3)
    h.read_g2o(path)                                                 # a file carries no kernels
    assert h.robust_kernel(1) == (0, 0.0)
    h.close()


def test_growth_after_a_prune_equals_a_fresh_graph(ctx, tmp_path):
    """Optimise, prune, append three nodes and a closure, optimise: the device copies and the structure are rebuilt, and the result
    is the one of a graph loaded from scratch with the same content, at the 1e-11 of the other incremental tests."""
    GM = capi.PG_ROBUST_GEMAN_MCCLURE
    g = _build(ctx, "130f", "d", lc_kernel=(GM, fx.MU))
    g.optimize(10)
    assert g.prune_edges(fx.PRUNE_THRESHOLD).tolist() == [fx.false_edge_index()]
    X = g.estimates()
    step = _mul7(_inv7(X[-2]), X[-1])
    last = X[-1]
    for _ in range(3):
        last = _mul7(last, step)
        g.augment_node(last)
    g.add_loop_closure(5, meas7=[0.01, 0, -0.02, 0, 0.01, 0, 1.0], info21=3 * np.eye(6))
    path = tmp_path / "grown.g2o"
    g.write_g2o(path)
    fresh = capi.PoseGraph(ctx)
    fresh.read_g2o(path, information=True)
    assert fresh.num_edges == g.num_edges
    for e in range(g.num_edges):
        kind, delta = g.robust_kernel(e)
        if kind:
            fresh.set_robust_kernel(e, kind, delta)
    assert sum(1 for e in range(g.num_edges) if g.robust_kernel(e)[0]) == 3
    cg, cf = g.optimize(5), fresh.optimize(5)
    d = np.abs(g.estimates() - fresh.estimates()).max()
    print(f"\nafter the prune and the growth: estimates differ by {d:.2e} from the graph loaded from scratch")
    assert cg[0] == pytest.approx(cf[0], rel=1e-12)
    assert d < 1e-11
    g.close()
    fresh.close()


def _robust_run(ctx, name, kind, delta):
    """ten iterations (what the fixture's first condition is stated for), the weights, the prune, two more iterations"""
    g = _build(ctx, name, "d", lc_kernel=(kind, delta))
    out = [g.optimize(10), g.estimates(), g.edge_residuals()[1], g.prune_edges(fx.PRUNE_THRESHOLD), g.optimize(2), g.estimates()]
    g.close()
    return out


def test_five_runs_are_identical(ctx):
    runs = [_robust_run(ctx, "130f", capi.PG_ROBUST_GEMAN_MCCLURE, fx.MU) for _ in range(5)]
    assert runs[0][3].tolist() == [fx.false_edge_index()]
    for r in runs[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(runs[0], r))


def test_two_graphs_on_one_context(ctx):
    """Two graphs with different kernels taking turns on one context give what each gives alone."""
    alone_a = _robust_run(ctx, "130f", capi.PG_ROBUST_GEMAN_MCCLURE, fx.MU)
    alone_b = _robust_run(ctx, "40", capi.PG_ROBUST_HUBER, 0.1)
    a = _build(ctx, "130f", "d", lc_kernel=(capi.PG_ROBUST_GEMAN_MCCLURE, fx.MU))
    b = _build(ctx, "40", "d", lc_kernel=(capi.PG_ROBUST_HUBER, 0.1))
    got_a, got_b = [], []
    for step in (lambda g: g.optimize(10), lambda g: g.estimates(), lambda g: g.edge_residuals()[1],
                 lambda g: g.prune_edges(fx.PRUNE_THRESHOLD), lambda g: g.optimize(2), lambda g: g.estimates()):
        got_a.append(step(a))
        got_b.append(step(b))
    a.close()
    b.close()
    assert all(np.array_equal(x, y) for x, y in zip(alone_a, got_a))
    assert all(np.array_equal(x, y) for x, y in zip(alone_b, got_b))


def test_global_optimize_removes_the_wrong_icp_closure(ctx):
    """PoseGraphOptimize.globalOptimize on the 40-vertex drifting loop: a 41st vertex placed so that the corner pair's registration T
    is its true closure to vertex 0, and the same registration hung on vertex 20 (across the circle: 1 m and 180 degrees away) as
    a deliberately wrong one.  The odometry edges carry 1000 I, the order of the closures' information (300 correspondences): with
    the identity there the arbiter's undamped Gauss-Newton itself diverges on this graph (steps of |dq| > 1 from the second
    iteration on, translations of kilometres by the tenth).  With 1000 I, on the arbiter (mu = 1.5^2 x 300): the wrong closure
    stays at w = 3.4e-6, the true one above 0.9996, the steps fall to 1e-15 by the tenth iteration, cond(H) = 6.5e5."""
    c, ref = ifx.cases()["corner_pair"], ifx.reference("corner_pair")
    z = capi.icp_meas7(ref["pair"][0])
    est = chain(40)[0]
    x40 = _mul7(est[0], _inv7(z))
    x40[0] += 0.02
    pg = capi.PoseGraph(ctx)
    for p in list(est[1:]) + [x40]:
        pg.augment_node(p)
    for e in range(pg.num_edges):
        pg.set_edge_information(e, 1000.0 * np.eye(6))
    pgo = registration.PoseGraphOptimize(ctx, pg)
    T, L, _ = pgo.addPoseToGraph(c["src"], c["tgt"], loopClosureNode=0)
    pgo.addPoseToGraph(c["src"], c["tgt"], loopClosureNode=20)
    assert [u[:2] for u in pgo.uncertain] == [(40, 0), (40, 20)] and pgo.uncertain[0][2] == L[5, 5]
    ne = pg.num_edges
    removed = pgo.globalOptimize()
    assert [u[:2] for u in removed] == [(40, 20)] and pg.num_edges == ne - 1
    assert [u[:2] for u in pgo.uncertain] == [(40, 0)]
    mu = 1.5 ** 2 * L[5, 5]
    assert pg.robust_kernel(ne - 2) == (capi.PG_ROBUST_GEMAN_MCCLURE, mu)
    chi2, w, _ = pg.edge_residuals()
    assert w[-1] > 0.99 and np.all(w[:-1] == 1)
    assert pgo.globalOptimize() == []
    pg.close()


def test_adaptor_smoke_runs_on_gpu(ctx, tmp_path):
    from test_pg_robust_abi import build_smoke

    exe = tmp_path / "pg_robust_smoke"
    build_smoke(exe)
    out = subprocess.run([str(exe), str(tmp_path / "out.txt")], capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert out.returncode == 0 and "pg robust smoke ok" in out.stdout, (out.returncode, out.stdout, out.stderr)
    removed, before, after = (int(x) for x in (tmp_path / "out.txt").read_text().split())
    assert (removed, before, after) == (12, 26, 25)
