"""GPU parity of the SE3 pose-graph Gauss-Newton (svo_pg_*) against the f64 CPU oracle.
Tolerance: estimates <= 1e-8 relative per Gauss-Newton iteration."""
import pathlib
import time

import numpy as np
import pytest

from pg_fixtures import drifting_loop
from ros_stereo_slam_amd import capi

pytestmark = pytest.mark.gpu
GOLDEN = pathlib.Path(__file__).parent / "golden" / "posegraph_loop40.npz"


def _build(cls_factory, est, closures):
    g = cls_factory()
    for i in range(1, len(est)):
        g.augment_node(est[i])
        for at, to in closures:
            if at == i:
                g.add_loop_closure(to)
    return g


def _close(a, b, tol):
    dq = np.minimum(np.abs(a[:, 3:] - b[:, 3:]), np.abs(a[:, 3:] + b[:, 3:])).max()
    return np.abs(a[:, :3] - b[:, :3]).max() <= tol * max(1.0, np.abs(b[:, :3]).max()) and dq <= tol


def test_a_chain_staged_in_one_call_is_the_chain_staged_node_by_node(ctx):
    """svo_pg_augment_nodes: the closure edge of node i (closure_from[i] >= 0) goes in BEFORE node i, as
    svo_pg_add_loop_closure + svo_pg_augment_node do one by one (the reference's staging order,
    src/optimizationStuff.cpp:3-15,58-63): the same vertices, edges, measurements and iterates."""
    gt, est = drifting_loop(120, laps=2, yaw_drift=5e-4)
    lc = np.full(len(est), -1, np.int32)
    lc[70], lc[119] = 9, 58
    a, b = capi.PoseGraph(ctx), capi.PoseGraph(ctx)
    for i in range(1, len(est)):
        if lc[i] >= 0:
            a.add_loop_closure(int(lc[i]))
        a.augment_node(est[i])
    b.augment_nodes(est[1:60], lc[1:60])                 # in two pieces: a chain is extended the same way
    b.augment_nodes(est[60:], lc[60:])
    assert a.num_vertices == b.num_vertices == len(est) and a.num_edges == b.num_edges == len(est) - 1 + 2
    for (i, j, z), (i2, j2, z2) in zip(a.edges(), b.edges()):
        assert (i, j) == (i2, j2) and np.array_equal(z, z2)
    assert np.array_equal(a.optimize(5), b.optimize(5)) and np.array_equal(a.estimates(), b.estimates())
    with pytest.raises(capi.SvoError):
        b.augment_nodes(est[1:3], np.array([500, -1], np.int32))     # a closure onto a vertex that does not exist
    a.close()
    b.close()


@pytest.mark.parametrize("n,laps,closures", [(40, 1, [(39, 0)]), (50, 1, [(48, 0), (49, 0)]),
                                             (200, 2, [(120, 20), (199, 99)])])
def test_iterates_match_oracle(ctx, orc, n, laps, closures):
    gt, est = drifting_loop(n, laps=laps, yaw_drift=1e-3 / laps)
    for iters in (1, 2, 4, 10):
        g = _build(lambda: capi.PoseGraph(ctx), est, closures)
        o = _build(orc.PoseGraph, est, closures)
        assert g.num_vertices == o.num_vertices and g.num_edges == o.num_edges
        for (a, b, z), (a2, b2, z2) in zip(g.edges(), o.edges()):
            assert (a, b) == (a2, b2) and np.abs(z - z2).max() < 1e-14
        cg, co = g.optimize(iters), o.optimize(iters)
        assert np.allclose(cg, co, rtol=1e-8, atol=1e-18), (iters, cg, co)
        assert _close(g.estimates(), o.estimates(), 1e-8), iters
        assert np.array_equal(g.estimates()[0], [0, 0, 0, 0, 0, 0, 1])
        g.close()


@pytest.mark.parametrize("cover", ["1", "0"])
@pytest.mark.parametrize("n,laps,closures", [(50, 1, [(48, 0), (49, 0)]), (215, 2, [(214, 107)])])
def test_refinement_passes_two_to_four(ctx, orc, monkeypatch, n, laps, closures, cover):
    """svo_pg_set_refinement(2 .. 4): the middle passes add their correction to the dx of the passes before IN PLACE
    (pg_backsub_update_kernel with dx_add == dx_out, neither of them __restrict__).  The iterates meet the oracle within
    test_iterates_match_oracle's tolerances, and the last chi2 is not above the one a single refinement pass reaches, within that
    tolerance.  50 vertices, two closures to the fixed vertex (no separator at all); a chain of 215, two laps, with one closure a
    lap back (regular separators; under the cover the closure's earlier endpoint stays inside a segment); both structures."""
    monkeypatch.setenv("SVO_PG_COVER", cover)
    gt, est = drifting_loop(n, laps=laps, yaw_drift=1e-3 / laps)
    for iters in (1, 2, 4, 10):
        o = _build(orc.PoseGraph, est, closures)
        co, eo = o.optimize(iters), o.estimates()
        last = {}
        for passes in (1, 2, 3, 4):
            g = _build(lambda: capi.PoseGraph(ctx), est, closures)
            g.set_refinement(passes)
            cg = g.optimize(iters)
            last[passes] = cg[-1]
            print(f"n {n} cover {cover} iters {iters} passes {passes}: chi2 {cg[-1]:.17g} (oracle {co[-1]:.17g}), "
                  f"estimates max |diff| {np.abs(g.estimates() - eo).max():.3e}")
            if passes >= 2:
                assert np.allclose(cg, co, rtol=1e-8, atol=1e-18), (iters, passes, cg, co)
                assert _close(g.estimates(), eo, 1e-8), (iters, passes)
                assert np.array_equal(g.estimates()[0], [0, 0, 0, 0, 0, 0, 1])
                assert cg[-1] <= last[1] + 1e-8 * abs(last[1]) + 1e-18, (iters, passes, cg[-1], last[1])
            g.close()


def test_awkward_segment_shapes(ctx, orc):
    """The elimination structure's corner cases in one graph of 760 vertices, four laps of a loop, every closure between
    true revisits (vertex i + 190 k and vertex i): runs of 0, 1, 2, 3, 13, 16, 17, 29, 64, 73, 74, 83 and 103 rows
    between separators (103: the longest a workgroup's LDS takes; every level count of the cyclic reduction from 1 to 7),
    separators next to each other, closures that share an endpoint, closures to the fixed vertex 0 and to vertex 1 (the
    first unknown), the first and the last unknown as separators."""
    gt, est = drifting_loop(760, radius=60.0, yaw_drift=2e-4, scale_drift=1.0005, laps=4)
    cuts = [1, 3, 6, 10, 12, 16, 33, 51, 116]
    closures = [(190 + c, c) for c in cuts] + [(410, 220), (571, 1), (192, 2), (190, 0), (380, 0), (675, 485), (759, 569)]
    closures.sort()
    ends = sorted({a - 1 for a, b in closures} | {b - 1 for a, b in closures if b > 0})
    runs = set(np.diff(ends) - 1)
    assert {0, 1, 2, 3, 13, 16, 17, 64, 73, 103} <= runs, sorted(runs)
    g = _build(lambda: capi.PoseGraph(ctx), est, closures)
    o = _build(orc.PoseGraph, est, closures)
    cg, co = g.optimize(6), o.optimize(6)
    assert cg[0] == pytest.approx(co[0], rel=1e-12)
    assert np.all(np.abs(cg[1:] - co[1:]) <= 1e-7 * co[:-1] + 1e-14), (cg, co)
    assert _close(g.estimates(), o.estimates(), 1e-7)
    assert cg[-1] < 1e-2 * cg[0]
    g.close()


def test_many_separators(ctx, orc):
    """3000 vertices, 75 closures with both endpoints spread over the laps: about 150 separators, a 19-tile separator system
    -- the tile steps, the separator solve's far blocks beyond the eight it keeps in flight, and the gather lists at a size
    the bench graph (11 tiles) does not reach."""
    gt, est = drifting_loop(3000, radius=200.0, yaw_drift=2e-5, scale_drift=1.0002, laps=5)
    rng = np.random.default_rng(11)
    at = sorted(rng.choice(np.arange(640, 3000), size=75, replace=False).tolist())
    closures = [(a, a - 600 * int(rng.integers(1, a // 600 + 1))) for a in at]
    closures = [(a, b) for a, b in closures if b >= 1]
    g = _build(lambda: capi.PoseGraph(ctx), est, closures)
    o = _build(orc.PoseGraph, est, closures)
    cg, co = g.optimize(5), o.optimize(5)
    assert cg[0] == pytest.approx(co[0], rel=1e-12)
    assert np.all(np.abs(cg[1:] - co[1:]) <= 1e-6 * co[:-1] + 1e-12), (cg, co)
    assert _close(g.estimates(), o.estimates(), 1e-6)
    assert cg[-1] < 1e-2 * cg[0]
    g.close()


def test_cover_structure(ctx, orc, monkeypatch):
    """SVO_PG_COVER=1: one endpoint per closure among the separators, the other inside a segment with a pass of six more
    right-hand-side columns (posegraph.hip, pg_segment_kernel).  Same answers as the oracle on the corner-case graph (closures
    that share endpoints, several closure endpoints inside one segment: the cap of eight (PG_MAX_SEG_CHORDS) is exceeded and re-covered) and on a
    graph whose matches all lie in the first lap."""
    monkeypatch.setenv("SVO_PG_COVER", "1")
    gt, est = drifting_loop(760, radius=60.0, yaw_drift=2e-4, scale_drift=1.0005, laps=4)
    cuts = [1, 3, 6, 10, 12, 16, 33, 51, 116]
    a = [(190 + c, c) for c in cuts] + [(410, 220), (571, 1), (192, 2), (190, 0), (380, 0), (675, 485), (759, 569)]
    b = [(200 + 40 * k + 190 * (k % 3), 10 + 40 * k) for k in range(4)] + [(700 + k, 130 + k) for k in (0, 7, 19, 31, 44)]
    for closures in (sorted(a), sorted(b)):
        g = _build(lambda: capi.PoseGraph(ctx), est, closures)
        o = _build(orc.PoseGraph, est, closures)
        cg, co = g.optimize(6), o.optimize(6)
        assert cg[0] == pytest.approx(co[0], rel=1e-12)
        assert np.all(np.abs(cg[1:] - co[1:]) <= 1e-7 * co[:-1] + 1e-14), (cg, co)
        assert _close(g.estimates(), o.estimates(), 1e-7)
        assert cg[-1] < 1e-2 * cg[0]
        g.close()


def test_golden_and_odometry_only(ctx):
    gt, est = drifting_loop(40)
    g = _build(lambda: capi.PoseGraph(ctx), est, [(39, 0)])
    gold = np.load(GOLDEN)
    assert np.abs(g.estimates() - gold["start"]).max() < 1e-12
    chi2 = g.optimize(4)
    assert np.allclose(chi2, gold["chi2"], rtol=1e-8, atol=1e-15)
    assert np.abs(g.estimates() - gold["after4"]).max() < 1e-8
    g.close()
    g = _build(lambda: capi.PoseGraph(ctx), est, [])
    before = g.estimates()
    chi2 = g.optimize(10)
    assert chi2.max() < 1e-20 and np.abs(g.estimates() - before).max() < 1e-12
    g.close()


@pytest.mark.parametrize("n_closures", [2, 40])
def test_kitti_sized_graph(ctx, orc, tmp_path, n_closures):
    """4541 vertices (KITTI 00) with closures spanning a whole lap: the oracle factorises in time
    order (long skyline rows), the GPU in nested-dissection order (35 regular separators + the
    closure endpoints, a dense Schur complement of up to 115 block rows)."""
    gt, est = drifting_loop(4541, radius=300.0, yaw_drift=1e-5, scale_drift=1.0001, laps=2)
    if n_closures == 2:
        closures = [(2400, 130), (4540, 2269)]  # revisits one lap (2270 vertices) later
    else:
        closures = [(2300 + 55 * k, 30 + 55 * k) for k in range(n_closures)]
    g = _build(lambda: capi.PoseGraph(ctx), est, closures)
    o = _build(orc.PoseGraph, est, closures)
    t0 = time.perf_counter()
    cg = g.optimize(10)
    tg = time.perf_counter() - t0
    t0 = time.perf_counter()
    co = o.optimize(10)
    to = time.perf_counter() - t0
    print(f"pose graph 4541 vertices, {n_closures} closures, 10 GN iterations: GPU {tg * 1e3:.1f} ms, "
          f"oracle {to * 1e3:.1f} ms")
    # a 4541-long chain is ill-conditioned (kappa ~ n^2): two exact factorisations in different
    # elimination orders give steps that agree to ~1e-6, so the chi2 after a step agrees to 1e-6 of
    # the chi2 the step STARTED from (each step removes 2-3 orders of magnitude), and both converge
    # to the same optimum
    assert cg[0] == pytest.approx(co[0], rel=1e-12)
    assert np.all(np.abs(cg[1:] - co[1:]) <= 1e-6 * co[:-1] + 1e-12)
    assert np.isclose(cg[-1], co[-1], rtol=1e-6, atol=1e-12)
    assert _close(g.estimates(), o.estimates(), 1e-6)
    assert cg[-1] < 1e-2 * cg[0]
    p = tmp_path / "poseGraph.g2o"
    g.write_g2o(p)
    lines = p.read_text().splitlines()
    assert sum(l.startswith("VERTEX_SE3:QUAT") for l in lines) == 4541
    assert sum(l.startswith("EDGE_SE3:QUAT") for l in lines) == 4540 + n_closures
    g.close()


def test_g2o_round_trip_and_fixture(ctx, orc, tmp_path):
    """svo_pg_read_g2o is the inverse of saveStructure's writer (poseGraph.h:140-179): a written
    graph read back optimises to the same chi2; a hand-written .g2o file (tests/golden) loads, its
    closed square is already consistent, and malformed files are refused."""
    gt, est = drifting_loop(60, radius=20.0, yaw_drift=2e-3, scale_drift=1.002, laps=1)
    g = _build(lambda: capi.PoseGraph(ctx), est, [(59, 0)])
    p = tmp_path / "a.g2o"
    g.write_g2o(p)
    h = capi.PoseGraph(ctx)
    h.read_g2o(p)
    assert h.num_vertices == g.num_vertices and h.num_edges == g.num_edges
    assert np.allclose(h.estimates(), g.estimates(), atol=1e-15)
    cg, ch = g.optimize(5), h.optimize(5)
    assert np.allclose(cg, ch, rtol=1e-9, atol=1e-18)
    assert _close(g.estimates(), h.estimates(), 1e-9)
    # the hand-written fixture: 4 vertices, 4 edges, a consistent square -> chi2 == 0 from the start
    f = capi.PoseGraph(ctx)
    f.read_g2o(pathlib.Path(__file__).parent / "golden" / "square4.g2o")
    assert f.num_vertices == 4 and f.num_edges == 4
    assert f.edges()[3][:2] == (3, 0)
    chi = f.optimize(3)
    assert chi.max() < 1e-24
    # a perturbed copy of it converges back
    est4 = f.estimates().copy()
    est4[2, :3] += [0.05, -0.02, 0.01]
    pert = tmp_path / "pert.g2o"
    lines = (pathlib.Path(__file__).parent / "golden" / "square4.g2o").read_text().splitlines()
    lines = [("VERTEX_SE3:QUAT 2 " + " ".join(repr(float(x)) for x in est4[2])) if l.startswith("VERTEX_SE3:QUAT 2 ") else l
             for l in lines]
    pert.write_text("\n".join(lines) + "\n")
    f.read_g2o(pert)
    chi = f.optimize(4)
    assert chi[0] > 1e-4 and chi[-1] < 1e-12 * chi[0] + 1e-20
    bad = tmp_path / "bad.g2o"
    bad.write_text("VERTEX_SE3:QUAT 0 0 0 0 0 0 0 1\nVERTEX_SE3:QUAT 2 1 0 0 0 0 0 1\n")   # id gap
    with pytest.raises(capi.SvoError):
        f.read_g2o(bad)
    bad.write_text("VERTEX_SE3:QUAT 0 0 0 0 0 0 0 1\nEDGE_SE3:QUAT 0 5 1 0 0 0 0 0 1\n")      # dangling edge
    with pytest.raises(capi.SvoError):
        f.read_g2o(bad)
    for x in (g, h, f):
        x.close()


def test_incremental_solves_equal_solves_from_scratch(ctx, orc, tmp_path):
    """The reference solves the whole graph again at every closure (src/VisualSLAM.cpp:76-86).  The
    device copy of the graph survives between solves: only appended vertices / edges are uploaded and
    the elimination structure is rebuilt only when the graph grew.  Each solve must equal -- to
    rounding -- the solve of a graph loaded from scratch (written out and read back before it), and follow
    the oracle driven through the same sequence."""
    gt, est = drifting_loop(300, laps=3, yaw_drift=4e-4)
    g, o = capi.PoseGraph(ctx), orc.PoseGraph()
    plan = {120: 19, 230: 128, 299: 97}          # frame -> LCidx, solved as soon as it is added
    for i in range(1, 300):
        if i in plan:
            g.add_loop_closure(plan[i])
            o.add_loop_closure(plan[i])
        g.augment_node(est[i])
        o.augment_node(est[i])
        if i in plan:
            path = tmp_path / f"before_{i}.g2o"
            g.write_g2o(path)
            fresh = capi.PoseGraph(ctx)
            fresh.read_g2o(path)                  # full upload, structure built from nothing
            cf = fresh.optimize(10)
            cg, co = g.optimize(10), o.optimize(10)
            # (reading a .g2o file re-normalises the quaternions: last-bit differences in the start values)
            assert np.allclose(cg, cf, rtol=1e-10, atol=1e-20) and np.abs(g.estimates() - fresh.estimates()).max() < 1e-11, i
            assert np.allclose(cg, co, rtol=1e-7, atol=1e-16)
            assert _close(g.estimates(), o.estimates(), 1e-7), i
            fresh.close()
            # a second solve without growth reuses the structure and the device copy as they are
            c2 = g.optimize(3)
            c2o = o.optimize(3)
            assert np.allclose(c2, c2o, rtol=1e-6, atol=1e-16) and _close(g.estimates(), o.estimates(), 1e-7)
    # a failed argument path leaves the graph usable; re-initialising drops the device copy
    g.ctx.lib.svo_pg_initialize(g._h)
    assert g.num_vertices == 1 and g.optimize(2).max() == 0
    g.augment_node(est[1])
    g.augment_node(est[2])
    g.augment_node(est[3])
    g.add_loop_closure(0)
    h = _build(lambda: capi.PoseGraph(ctx), est[:4], [(3, 0)])
    assert np.array_equal(g.optimize(5), h.optimize(5)) and np.array_equal(g.estimates(), h.estimates())
    g.close()
    h.close()


# ---- the arbiter: which of the two factorisations is the accurate one? ----
def _bench_like_graph(V=4541, n_closures=40):
    """BASELINE configs[2]'s graph as tools/pg_profile.py builds it: the bench loop with a random-walk drift, the
    generator's revisits as closures"""
    from ros_stereo_slam_amd import chunked, synth

    poses = synth.loop_trajectory(V, **synth.BENCH_LOOP)
    R0, t0 = poses[0]
    rng = np.random.default_rng(1)
    est, drift = [], np.zeros(3)
    for R, t in poses:
        drift = drift + rng.normal(0, 0.002, 3)
        est.append(chunked.pose7(R0.T @ R, R0.T @ (t - t0) + drift))
    matches = synth.loop_closures(poses, max_dist=0.3, max_angle_deg=10.0, min_gap=100, pick="nearest")
    cl = list(chunked.gate_closures([m if m >= 1 else -1 for m in matches]).items())[:n_closures]
    return est, [(q, max(m - 1, 0)) for q, m in cl]


def _many_separators_graph():
    gt, est = drifting_loop(3000, radius=200.0, yaw_drift=2e-5, scale_drift=1.0002, laps=5)
    rng = np.random.default_rng(11)
    at = sorted(rng.choice(np.arange(640, 3000), size=75, replace=False).tolist())
    closures = [(a, a - 600 * int(rng.integers(1, a // 600 + 1))) for a in at]
    return est, [(a, b) for a, b in closures if b >= 1]


@pytest.mark.parametrize("which", ["bench 4541 / 40", "3000 / 75", "760 corner cases"])
def test_gpu_iterates_against_the_refined_arbiter(ctx, orc, which):
    """Every Gauss-Newton iteration, from the graph's OWN estimates: the GPU's iterate against the step of the same normal
    equations solved by a sparse LU + iterative refinement with 80-bit residuals (tests/pg_arbiter.py), and the oracle's
    against the same arbiter.  SURVEY.md 8d's 1e-8 is asserted for the GPU against the ARBITER; where the time-ordered
    oracle is further from the arbiter than that, the GPU-vs-oracle tests above carry a looser bound because of the
    ORACLE's factorisation, and this test says so with numbers."""
    import pg_arbiter as arb

    if which.startswith("bench"):
        est, closures = _bench_like_graph()
        iters = 4
    elif which.startswith("3000"):
        est, closures = _many_separators_graph()
        iters = 4
    else:
        gt, est = drifting_loop(760, radius=60.0, yaw_drift=2e-4, scale_drift=1.0005, laps=4)
        cuts = [1, 3, 6, 10, 12, 16, 33, 51, 116]
        closures = sorted([(190 + c, c) for c in cuts] + [(410, 220), (571, 1), (192, 2), (190, 0), (380, 0), (675, 485), (759, 569)])
        iters = 5
    g = _build(lambda: capi.PoseGraph(ctx), est, closures)
    r = _build(lambda: capi.PoseGraph(ctx), est, closures)
    r.set_refinement(1)
    o = _build(orc.PoseGraph, est, closures)
    print(f"\n{which}: {len(est)} vertices, {len(closures)} closures")
    print(" GPU (nested dissection, block cyclic reduction, f64 MFMA tiles), one solve per step, against the arbiter:")
    dg = arb.compare_iterates(g, iters, log=print)
    print(" GPU with one refinement pass (svo_pg_set_refinement(1): the residual in double-double, the same elimination again):")
    dr = arb.compare_iterates(r, iters, log=print)
    print(" oracle (time-ordered skyline Cholesky) against the arbiter:")
    do = arb.compare_iterates(o, iters, log=print)
    # the refined run's final estimates equal the single-solve run's to the solver's accuracy (the same minimum)
    final = arb.deviation(g.estimates(), r.estimates())
    g.close()
    r.close()
    worst = lambda d: max(max(x) for x in d)   # noqa: E731
    print(f" worst over the iterations: GPU {worst(dg):.2e}, GPU refined {worst(dr):.2e}, oracle {worst(do):.2e}; "
          f"single-solve vs refined estimates after {iters} iterations {max(final):.2e}")
    for k, (dt, dq) in enumerate(dr):
        assert dt <= 1e-8 and dq <= 1e-8, (which, "refined", k, dt, dq)        # SURVEY.md 8d's bound, against the arbiter
    for k, (dt, dq) in enumerate(dg):
        assert dt <= 5e-8 and dq <= 5e-8, (which, "single solve", k, dt, dq)   # cond(H) ~ 1e8: what ONE f64 solve can give
    assert worst(dg) <= worst(do) * 1.5 or worst(dg) <= 1e-9                   # never less accurate than the time-ordered oracle
    assert max(final) <= 1e-7


@pytest.mark.parametrize("n", list(range(101, 112)) + list(range(206, 216)) + [312, 313, 314])
def test_tail_segments_around_the_regular_separator_spacing(ctx, orc, n):
    """Chains whose length sits around a multiple of the regular separator spacing (104 rows): the run after the last
    separator is 102 ... 105 rows long -- 104 is the longest segment a workgroup's LDS is sized for (the
    regular-separator loop stops one row early, the static_assert checked 103).  One closure to the fixed vertex, one
    near the start."""
    gt, est = drifting_loop(n, laps=1, yaw_drift=2e-3)
    for closures in ([(n - 1, 0)], [(n - 1, 0), (n - 2, 1)], []):
        g = _build(lambda: capi.PoseGraph(ctx), est, closures)
        o = _build(orc.PoseGraph, est, closures)
        cg, co = g.optimize(3), o.optimize(3)
        assert np.allclose(cg, co, rtol=1e-8, atol=1e-18), (n, closures, cg, co)
        assert _close(g.estimates(), o.estimates(), 1e-8), (n, closures)
        g.close()
