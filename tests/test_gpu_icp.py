"""svo_cloud and the ICP entry points on the GPU, bit for bit against the numpy restatement (tests/icp_numpy.py) on every
fixture of tests/icp_fixtures.py: correspondences, neighbour lists, normals, one step's normal equations, whole
registrations, the information matrix and the pairwise registration; memory modes, repeatability, svo_sor_filter_large
next to a cloud, the error paths, and a measured closure hung on a pose graph."""
import ctypes as C

import numpy as np
import pytest

import icp_fixtures as fx
import pg_info_fixtures as pif
from ros_stereo_slam_amd import capi, registration

pytestmark = pytest.mark.gpu
NAMES = sorted(fx.cases())


@pytest.fixture(scope="module")
def clouds(ctx):
    """name -> Cloud with estimated normals, built once"""
    out = {}
    for name, c in fx.cases().items():
        out[name] = capi.Cloud(ctx, c["tgt"]).estimate_normals(c["knn"])
    yield out
    for cl in out.values():
        cl.close()


@pytest.mark.parametrize("name", NAMES)
def test_correspondences(ctx, clouds, name):
    c, r = fx.cases()[name], fx.reference(name)
    corr, fit, rmse = ctx.icp_correspondences(c["src"], clouds[name], c["max_dist"], c["T"])
    assert np.array_equal(corr, r["corr"])
    assert fit == r["fitness"] and rmse == r["rmse"]


@pytest.mark.parametrize("name", NAMES)
def test_knn_and_normals(ctx, clouds, name):
    c, r = fx.cases()[name], fx.reference(name)
    assert len(clouds[name]) == len(c["tgt"])
    assert np.array_equal(clouds[name].knn(c["knn"]), r["knn"])
    assert np.array_equal(clouds[name].normals(), r["normals"])


@pytest.mark.parametrize("name", NAMES)
def test_one_step(ctx, clouds, name):
    c, r = fx.cases()[name], fx.reference(name)
    A, b, n = ctx.icp_normal_equations(c["src"], clouds[name], c["max_dist"], c["T"])
    assert n == r["n_corr_step"]
    assert np.array_equal(A, r["JtJ"]) and np.array_equal(b, r["Jtr"])


@pytest.mark.parametrize("name", NAMES)
def test_whole_icp(ctx, clouds, name):
    c, r = fx.cases()[name], fx.reference(name)
    T, fit, rmse, its, corr = ctx.icp_point_to_plane(c["src"], clouds[name], c["max_dist"], c["T"], want_corr=True)
    Tr, fr, rr, ir, cr = r["icp"]
    assert its == ir
    assert np.array_equal(T, Tr) and fit == fr and rmse == rr
    assert np.array_equal(corr, cr)


@pytest.mark.parametrize("name", NAMES)
def test_information(ctx, clouds, name):
    c, r = fx.cases()[name], fx.reference(name)
    L, n = ctx.icp_information(c["src"], clouds[name], c["max_dist"], c["T"])
    assert n == r["n_corr"] and np.array_equal(L, r["info"])


@pytest.mark.parametrize("name", NAMES)
def test_pairwise(ctx, clouds, name):
    c, r = fx.cases()[name], fx.reference(name)
    T, L, d = ctx.icp_pairwise(c["src"], clouds[name], *c["pair"])
    Tr, Lr, coarse, fine, n = r["pair"]
    assert list(d["iterations"]) == [coarse[3], fine[3]]
    assert np.array_equal(T, Tr) and np.array_equal(L, Lr) and d["n_corr"] == n
    assert list(d["fitness"]) == [coarse[1], fine[1]] and list(d["rmse"]) == [coarse[2], fine[2]]


def test_information_needs_no_normals(ctx):
    c, r = fx.cases()["corner_pair"], fx.reference("corner_pair")
    cl = capi.Cloud(ctx, c["tgt"])
    assert not cl.has_normals
    L, n = ctx.icp_information(c["src"], cl, c["max_dist"], c["T"])
    assert n == r["n_corr"] and np.array_equal(L, r["info"])
    cl.set_normals(r["normals"])
    assert np.array_equal(cl.normals(), r["normals"])
    assert np.array_equal(ctx.icp_point_to_plane(c["src"], cl, c["max_dist"], c["T"])[0], r["icp"][0])
    cl.close()


def test_device_memory_gives_the_same_bytes(ctx, clouds):
    import torch

    c, r = fx.cases()["corner_pair"], fx.reference("corner_pair")
    dev = torch.device("cuda", 0)
    src_d, tgt_d = torch.from_numpy(c["src"]).to(dev), torch.from_numpy(c["tgt"]).to(dev)
    cl = capi.Cloud(ctx, tgt_d).estimate_normals(c["knn"])
    assert np.array_equal(cl.normals(), r["normals"])
    T, fit, rmse, its, corr = ctx.icp_point_to_plane(src_d, cl, c["max_dist"], c["T"], want_corr=True)
    ctx.sync()
    assert np.array_equal(T, r["icp"][0]) and (fit, rmse, its) == r["icp"][1:4]
    assert np.array_equal(corr.cpu().numpy(), r["icp"][4])
    Tp, Lp, _ = ctx.icp_pairwise(src_d, cl, *c["pair"])
    assert np.array_equal(Tp, r["pair"][0]) and np.array_equal(Lp, r["pair"][1])
    cl.close()


def test_five_runs_are_identical(ctx, clouds):
    c = fx.cases()["corner_pair"]
    runs = [ctx.icp_pairwise(c["src"], clouds["corner_pair"], *c["pair"]) for _ in range(5)]
    for T, L, d in runs[1:]:
        assert T.tobytes() == runs[0][0].tobytes() and L.tobytes() == runs[0][1].tobytes()
        assert d["rmse"].tobytes() == runs[0][2]["rmse"].tobytes()


def test_sor_large_keeps_its_bits_next_to_a_cloud(ctx):
    rng = np.random.default_rng(4)
    xyz = np.concatenate([fx.corner(4097, step=0.125), (10 + 8 * rng.random((300, 3))).astype(np.float32)])
    a = ctx.sor_filter_large(xyz)
    cl = capi.Cloud(ctx, xyz).estimate_normals(30)
    ctx.icp_pairwise(fx.corner_source(300), cl)
    b = ctx.sor_filter_large(xyz)
    cl.close()
    assert a[0].tobytes() == b[0].tobytes() and a[2].tobytes() == b[2].tobytes()
    assert 0 < len(a[0]) < len(xyz)


def test_error_paths(ctx, clouds):
    c = fx.cases()["corner_pair"]
    with pytest.raises(capi.SvoError) as e:
        capi.Cloud(ctx, np.zeros((0, 3), np.float32))
    assert e.value.code == capi.SVO_ERR_ARG
    bad = c["tgt"].copy()
    bad[700, 1] = np.nan
    bad[900, 2] = np.inf
    with pytest.raises(capi.SvoError) as e:
        capi.Cloud(ctx, bad)
    assert e.value.code == capi.SVO_ERR_ARG and "point 700 " in str(e.value)
    cl = capi.Cloud(ctx, c["tgt"])
    for k in (2, 65):
        with pytest.raises(capi.SvoError) as e:
            cl.estimate_normals(k)
        assert e.value.code == capi.SVO_ERR_ARG
        with pytest.raises(capi.SvoError) as e:
            cl.knn(k)
        assert e.value.code == capi.SVO_ERR_ARG
    for call in (lambda: ctx.icp_point_to_plane(c["src"], cl, 1.5), lambda: ctx.icp_pairwise(c["src"], cl),
                 lambda: ctx.icp_normal_equations(c["src"], cl, 1.5), lambda: cl.normals()):
        with pytest.raises(capi.SvoError) as e:
            call()
        assert e.value.code == capi.SVO_ERR_STATE
    cl.close()
    for md in (0.0, -1.0, float("nan")):
        with pytest.raises(capi.SvoError) as e:
            ctx.icp_point_to_plane(c["src"], clouds["corner_pair"], md)
        assert e.value.code == capi.SVO_ERR_ARG
        with pytest.raises(capi.SvoError) as e:
            ctx.icp_information(c["src"], clouds["corner_pair"], md)
        assert e.value.code == capi.SVO_ERR_ARG
    with pytest.raises(capi.SvoError) as e:
        ctx.icp_point_to_plane(np.zeros((0, 3), np.float32), clouds["corner_pair"], 1.5)
    assert e.value.code == capi.SVO_ERR_ARG
    with pytest.raises(capi.SvoError) as e:
        ctx.icp_point_to_plane(c["src"], clouds["corner_pair"], 1.5, max_iteration=0)
    assert e.value.code == capi.SVO_ERR_ARG


def test_closure_from_icp_on_a_graph(ctx):
    """PoseGraphOptimize.addPoseToGraph hangs the corner pair's registration on the 40-vertex drifting loop as the closure
    (newest vertex -> vertex 0); the graph stores Omega, and the weighted solve lowers chi2 in its first iteration."""
    c, r = fx.cases()["corner_pair"], fx.reference("corner_pair")
    est, _ = pif.chain(40)
    pg = capi.PoseGraph(ctx)
    for p in est[1:]:
        pg.augment_node(p)
    ne = pg.num_edges
    pgo = registration.PoseGraphOptimize(ctx, pg)
    assert (pgo.max_correspondence_distance_coarse, pgo.max_correspondence_distance_fine) == (15, 1.5)
    T, L, info21 = pgo.addPoseToGraph(c["src"], c["tgt"], loopClosureNode=0)
    assert np.array_equal(T, r["pair"][0]) and np.array_equal(L, r["pair"][1])
    assert pg.num_edges == ne + 1
    a, b, z = pg.edges()[ne]
    assert (a, b) == (39, 0) and np.allclose(z, capi.icp_meas7(T), atol=1e-15)
    assert np.array_equal(pg.edge_information(ne), info21)
    assert np.array_equal(info21, capi.icp_edge_information(L, T))
    assert np.linalg.eigvalsh(capi.info_matrix(info21)).min() > 0
    chi2 = pg.optimize(3)
    assert np.all(np.isfinite(chi2)) and chi2[1] <= chi2[0]
    pg.close()
