"""Per-edge information matrices and measured loop closures of the pose graph (svo_pg_add_loop_closure_measured,
svo_pg_set_edge_information, svo_pg_read_g2o_info) on the GPU, against the weighted arbiter (tests/pg_info_arbiter.py:
sparse LU + refinement with 80-bit residuals on the oracle's edge linearisation).  SURVEY.md 8d's bound, 1e-8 per
Gauss-Newton iteration, is asserted against that arbiter."""
import numpy as np
import pytest

import pg_info_arbiter as arb
from pg_fixtures import drifting_loop
from pg_info_fixtures import GRAPHS, chain, edge_list, omega_set, rms_translation, square_lap, tri21
from ros_stereo_slam_amd import capi

pytestmark = pytest.mark.gpu
ID7 = np.array([0, 0, 0, 0, 0, 0, 1.0])


def _build(ctx, est, closures, omegas=None, measured=False, meas=None):
    """the chain node by node; closures through the old call, or (measured) through svo_pg_add_loop_closure_measured"""
    g = capi.PoseGraph(ctx)
    for i in range(1, len(est)):
        g.augment_node(est[i])
        for at, to in closures:
            if at == i:
                if measured:
                    g.add_loop_closure(to, meas7=ID7 if meas is None else meas)
                else:
                    g.add_loop_closure(to)
    if omegas is not None:
        assert len(omegas) == g.num_edges
        for e, Om in enumerate(omegas):
            g.set_edge_information(e, Om)
    return g


@pytest.mark.parametrize("V", sorted(GRAPHS))
def test_identity_information_changes_no_bit(ctx, V):
    """A graph built with the new calls but identity everywhere -- measured closures with the identity measurement, the
    identity set as every edge's information -- takes the identity kernel: the same bits as today's calls."""
    est, closures = chain(V)
    a = _build(ctx, est, closures)
    b = _build(ctx, est, closures, omegas=[np.eye(6)] * (V - 1 + len(closures)), measured=True)
    for (i, j, z), (i2, j2, z2) in zip(a.edges(), b.edges()):
        assert (i, j) == (i2, j2) and np.array_equal(z, z2)
    assert np.array_equal(b.edge_information(0), tri21(np.eye(6)))
    for k in range(1, 5):
        ca, cb = a.optimize(1), b.optimize(1)
        assert np.array_equal(ca, cb), k
        assert np.array_equal(a.estimates(), b.estimates()), k
    a.close()
    b.close()
    a = _build(ctx, est, closures)
    b = _build(ctx, est, closures, omegas=[None] * (V - 1 + len(closures)), measured=True)
    assert np.array_equal(a.optimize(4), b.optimize(4)) and np.array_equal(a.estimates(), b.estimates())
    a.close()
    b.close()


@pytest.mark.parametrize("V", sorted(GRAPHS))
def test_a_common_scale_scales_chi2_only(ctx, V):
    """4 I on every edge: the same minimiser, chi2 four times as large.  The two runs differ by the code shape of the two
    linearisations only: cond(H) eps ~ 1e5 * 1e-16 leaves four decades below the 1e-9 asked of the estimates."""
    est, closures = chain(V)
    edges = edge_list(est, closures)
    u = _build(ctx, est, closures)
    w = _build(ctx, est, closures, omegas=omega_set("s", edges))
    cu, cw = u.optimize(4), w.optimize(4)
    rel = np.abs(cw - 4 * cu) / (4 * cu)
    dev = arb.deviation(w.estimates(), u.estimates())
    print(f"\nV = {V}: chi2 {cu} -> x4 relative difference {rel}, estimates {dev}")
    assert np.all(rel <= 1e-12), (cu, cw)
    assert max(dev) <= 1e-9
    u.close()
    w.close()


@pytest.mark.parametrize("kind", ["d", "f"])
@pytest.mark.parametrize("V", sorted(GRAPHS))
def test_weighted_iterates_against_the_arbiter(ctx, V, kind):
    """Four Gauss-Newton iterations one at a time, each from the graph's own estimates, against the weighted arbiter's step.
    With one refinement pass: 1e-8.  The single solve: never further from the arbiter than 1.5 times what ONE
    plain float64 Cholesky factorisation (numpy, time order) of the arbiter's own H dx = b is, or 1e-9.

    Measured on an MI355X (worst of the four iterations; GPU single solve / numpy Cholesky / GPU refined):
      40 d 5.5e-14 / 5.9e-15 / 8.9e-15    40 f 6.0e-15 / 3.0e-15 / 1.2e-15
     130 d 1.0e-12 / 4.7e-13 / 4.8e-14   130 f 7.5e-14 / 6.2e-14 / 2.2e-14
     313 d 4.9e-12 / 8.9e-13 / 2.7e-13   313 f 4.9e-13 / 1.0e-13 / 5.8e-14
    The GPU's single solve is up to five times numpy's on these well-conditioned graphs (cond(H) <= 5.6e6) and more than two
    decades below 1e-9."""
    est, closures = chain(V)
    omegas = omega_set(kind, edge_list(est, closures))
    g = _build(ctx, est, closures, omegas=omegas)
    r = _build(ctx, est, closures, omegas=omegas)
    r.set_refinement(1)
    edges = g.edges()
    dev_g, dev_c, dev_r = [], [], []
    for k in range(4):
        X0 = g.estimates()
        g.optimize(1)
        Xa, dx, info = arb.step(X0, edges, omegas)
        dev_g.append(max(arb.deviation(g.estimates(), Xa)))
        dev_c.append(max(arb.deviation(arb.plain_cholesky_step(X0, info), Xa)))
        X0 = r.estimates()
        r.optimize(1)
        Xa, dx, info = arb.step(X0, edges, omegas)
        dev_r.append(max(arb.deviation(r.estimates(), Xa)))
    print(f"\nV = {V}, set {kind}: deviation from the arbiter per iteration: GPU single solve {['%.1e' % d for d in dev_g]}, "
          f"numpy Cholesky {['%.1e' % d for d in dev_c]}, GPU refined {['%.1e' % d for d in dev_r]}")
    g.close()
    r.close()
    assert max(dev_r) <= 1e-8, dev_r
    assert max(dev_g) <= 1.5 * max(dev_c) or max(dev_g) <= 1e-9, (dev_g, dev_c)


def _closure_error_norm(orc, X, edge):
    i, j, z = edge
    return float(np.linalg.norm(orc.se3_edge_error(X[i], X[j], z)[0]))


def test_weights_act(ctx, orc):
    """40 vertices, ten iterations, odometry at I: with the closure at 100 I its final error is smaller than with the closure
    at 0.01 I, by at least the factor the arbiter gives for the same two runs, less 1 %."""
    est, closures = chain(40)
    n_e = 39 + 1
    ce = [k for k, (_, _, c) in enumerate(edge_list(est, closures)) if c][0]
    norms_g, norms_a = {}, {}
    for wgt in (100.0, 0.01):
        omegas = [np.eye(6)] * n_e
        omegas[ce] = wgt * np.eye(6)
        g = _build(ctx, est, closures, omegas=omegas)
        edges, X0 = g.edges(), g.estimates()
        g.optimize(10)
        Xg = g.estimates()
        g.close()
        Xa = arb.optimize(X0, edges, omegas, iters=10)
        assert max(arb.deviation(Xg, Xa)) <= 1e-8, wgt
        norms_g[wgt] = _closure_error_norm(orc, Xg, edges[ce])
        norms_a[wgt] = _closure_error_norm(orc, Xa, edges[ce])
    factor_g, factor_a = norms_g[0.01] / norms_g[100.0], norms_a[0.01] / norms_a[100.0]
    print(f"\nclosure |e| at 0.01 I / at 100 I: GPU {factor_g:.6g}, arbiter {factor_a:.6g}")
    assert factor_a > 10
    assert factor_g >= 0.99 * factor_a


def test_measured_closure(ctx):
    """A square lap of 40 poses whose last pose is 0.4 m and 5 degrees off pose 0, odometry with a seeded yaw drift: the
    closure that carries the measured X39^-1 X0 brings the lap closer to the ground truth than the identity closure, by at
    least the factor the arbiter gives for the same two runs, less 1 %."""
    gt, est, meas = square_lap(40, drift_seed=0)
    rms_g, rms_a = {}, {}
    for name, z in (("identity", None), ("measured", meas)):
        g = capi.PoseGraph(ctx)
        for i in range(1, len(est)):
            g.augment_node(est[i])
        g.add_loop_closure(0, meas7=z)
        edges, X0 = g.edges(), g.estimates()
        assert np.allclose(edges[-1][2], ID7 if z is None else z, atol=1e-15)
        g.optimize(10)
        Xg = g.estimates()
        g.close()
        Xa = arb.optimize(X0, edges, None, iters=10)
        assert max(arb.deviation(Xg, Xa)) <= 1e-8, name
        rms_g[name], rms_a[name] = rms_translation(Xg, gt), rms_translation(Xa, gt)
    factor_g, factor_a = rms_g["identity"] / rms_g["measured"], rms_a["identity"] / rms_a["measured"]
    print(f"\nRMS translation error: identity {rms_g['identity']:.4f} m, measured {rms_g['measured']:.4f} m: "
          f"factor GPU {factor_g:.6g}, arbiter {factor_a:.6g}")
    assert factor_a > 1
    assert factor_g >= 0.99 * factor_a


@pytest.mark.parametrize("start_weighted", [False, True])
def test_incremental_information(ctx, tmp_path, start_weighted):
    """Optimise; change the information of an edge the device already holds and append three nodes (one of them with a
    weighted measured closure); optimise again: the information buffer is uploaded again, the appended edges are appended,
    and the result is the one of a graph loaded from scratch with the same content (the bound of the unweighted
    incremental test: reading a .g2o file re-normalises the quaternions, last-bit differences in the start values)."""
    est_all = np.array(drifting_loop(44, laps=2, yaw_drift=1e-3)[1])   # a lap is 22 vertices: 40 revisits 18, 42 revisits 20
    est = est_all[:41]
    closures = [(40, 18)]
    edges = edge_list(est, closures)
    g = _build(ctx, est, closures, omegas=omega_set("f", edges) if start_weighted else None)
    g.optimize(3)
    Q = omega_set("f", edges, seed=77)
    g.set_edge_information(7, Q[7])
    g.augment_node(est_all[41])
    g.augment_node(est_all[42])
    g.add_loop_closure(20, meas7=[0.01, 0, -0.02, 0, 0.01, 0, 1.0], info21=Q[3])
    g.augment_node(est_all[43])
    assert np.array_equal(g.edge_information(7), tri21(Q[7]))
    assert np.array_equal(g.edge_information(g.num_edges - 2), tri21(Q[3]))
    assert np.array_equal(g.edge_information(g.num_edges - 1), tri21(np.eye(6)))
    path = tmp_path / "before.g2o"
    g.write_g2o(path)
    fresh = capi.PoseGraph(ctx)
    fresh.read_g2o(path, information=True)
    assert fresh.num_edges == g.num_edges
    for e in range(g.num_edges):
        assert np.array_equal(fresh.edge_information(e), g.edge_information(e))
    cg, cf = g.optimize(5), fresh.optimize(5)
    print(f"\nchi2 after the change: {cg}; against the graph loaded from scratch: chi2 relative {np.abs(cg - cf) / cf}, "
          f"estimates {np.abs(g.estimates() - fresh.estimates()).max():.2e}")
    assert cg[-1] < cg[0]
    # The estimates: 1e-11, the bound of the unweighted incremental test.  chi2: the two runs start from values that differ
    # in the last bit and a step removes one to two decades of chi2, so what a step's rounding leaves shows against the chi2
    # the step STARTED from (the form of test_gpu_posegraph.py's comparisons of chi2 sequences), at that test's 1e-10.
    assert cg[0] == pytest.approx(cf[0], rel=1e-12)
    assert np.all(np.abs(cg[1:] - cf[1:]) <= 1e-10 * cf[:-1]), (cg, cf)
    assert np.abs(g.estimates() - fresh.estimates()).max() < 1e-11
    # resetting every edge brings the identity kernel back: the unweighted graph
    for e in range(g.num_edges):
        g.set_edge_information(e, None)
    reset = tmp_path / "reset.g2o"
    g.write_g2o(reset)
    plain = capi.PoseGraph(ctx)
    plain.read_g2o(reset)
    assert np.allclose(g.optimize(2), plain.optimize(2), rtol=1e-10, atol=1e-20)
    assert np.abs(g.estimates() - plain.estimates()).max() < 1e-11
    for x in (g, fresh, plain):
        x.close()


def _identity_tail():
    return "".join(" %d" % (1 if i == j else 0) for i in range(6) for j in range(i, 6))


def test_file_format(ctx, tmp_path):
    est, closures = chain(40)
    edges = edge_list(est, closures)
    omegas = omega_set("f", edges)
    omegas[5] = None                        # one edge without stored information among the others
    g = _build(ctx, est, closures, omegas=omegas)
    path = tmp_path / "w.g2o"
    g.write_g2o(path)
    h = capi.PoseGraph(ctx)
    h.read_g2o(path, information=True)
    assert h.num_edges == g.num_edges
    for e in range(g.num_edges):
        want = tri21(np.eye(6) if omegas[e] is None else omegas[e])
        assert np.array_equal(g.edge_information(e), want) and np.array_equal(h.edge_information(e), want), e
    lines = [l for l in path.read_text().splitlines() if l.startswith("EDGE_SE3:QUAT")]
    assert lines[5].endswith(_identity_tail())
    assert np.allclose(g.optimize(4), h.optimize(4), rtol=1e-10, atol=1e-20)
    # svo_pg_read_g2o on the same file: the information is ignored, the unweighted graph
    u = capi.PoseGraph(ctx)
    u.read_g2o(path)
    p = _build(ctx, est, closures)
    for e in range(u.num_edges):
        assert np.array_equal(u.edge_information(e), tri21(np.eye(6)))
    cu, cp = u.optimize(4), p.optimize(4)
    assert np.allclose(cu, cp, rtol=1e-10, atol=1e-20) and np.abs(u.estimates() - p.estimates()).max() < 1e-11
    # a graph without stored information writes the bytes it always wrote
    q = _build(ctx, est, closures)
    plain = tmp_path / "plain.g2o"
    q.write_g2o(plain)
    X, want = q.estimates(), ""
    for v in range(len(X)):
        want += "VERTEX_SE3:QUAT %d " % v + " ".join("%.17g" % x for x in X[v]) + "\n"
    for (i, j, z) in q.edges():
        want += "EDGE_SE3:QUAT %d %d " % (i, j) + " ".join("%.17g" % x for x in z) + _identity_tail() + "\n"
    assert plain.read_bytes() == want.encode()
    # 20 information numbers: refused with the line number
    bad = tmp_path / "bad.g2o"
    good = path.read_text().splitlines()
    k = next(n for n, l in enumerate(good) if l.startswith("EDGE_SE3:QUAT"))
    good[k] = " ".join(good[k].split()[:-1])
    bad.write_text("\n".join(good) + "\n")
    with pytest.raises(capi.SvoError) as ei:
        h.read_g2o(bad, information=True)
    assert ei.value.code == capi.SVO_ERR_ARG and f":{k + 1}:" in str(ei.value)
    h.read_g2o(bad)                         # the reader that ignores the information takes the line
    # matrices that are no information matrices: refused, the graph unchanged
    rng = np.random.default_rng(4)
    Qr, _ = np.linalg.qr(rng.normal(size=(6, 6)))
    zero_diag = np.diag([1, 1, 0, 1, 1, 1.0])
    indefinite = Qr @ np.diag([1, 1, 1, 1, 1, -1.0]) @ Qr.T
    nan = np.eye(6)
    nan[2, 4] = nan[4, 2] = np.nan
    before = [g.edge_information(e) for e in range(g.num_edges)]
    ne, X = g.num_edges, g.estimates()
    for M in (zero_diag, (indefinite + indefinite.T) / 2, nan):
        with pytest.raises(capi.SvoError) as ei:
            g.set_edge_information(3, M)
        assert ei.value.code == capi.SVO_ERR_ARG and "edge 3" in str(ei.value)
        with pytest.raises(capi.SvoError) as ei:
            g.add_loop_closure(1, meas7=ID7, info21=M)
        assert ei.value.code == capi.SVO_ERR_ARG
        assert g.num_edges == ne and np.array_equal(g.estimates(), X)
        assert all(np.array_equal(g.edge_information(e), before[e]) for e in range(ne))
    for x in (g, h, u, p, q):
        x.close()
