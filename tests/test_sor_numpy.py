"""The restatement of svo_sor_filter_large (tests/sor_numpy.py) against the oracle of visualSLAM::SORcloud and the
dense numpy restatement of test_oracle_sor, bit for bit, and against hand-computed answers."""
import numpy as np
import pytest

import sor_numpy as sn
from test_oracle_sor import cloud, numpy_sor


@pytest.mark.parametrize("n", [1, 2, 3, 150, 1000, 3000])
@pytest.mark.parametrize("k", [1, 20, 200])
@pytest.mark.parametrize("z_limit", [0.0, 60.0])
def test_matches_oracle(orc, n, k, z_limit):
    xyz, col = cloud(n, seed=7 * n + k, outliers=n // 40)
    xo, co, mo = orc.sor_filter(xyz, col, mean_k=k, stddev_mul=0.8, z_limit=z_limit)
    xs, cs, ms = sn.sor_filter(xyz, col, mean_k=k, stddev_mul=0.8, z_limit=z_limit)
    assert np.array_equal(ms, mo)
    assert np.array_equal(xs, xo) and np.array_equal(cs, co)


@pytest.mark.parametrize("k", [1, 20, 200])
def test_duplicates_match_oracle(orc, k):
    xyz, col = cloud(700, seed=11)
    xyz = np.concatenate([xyz, xyz[:300], xyz[:300], np.repeat(xyz[5:6], 250, axis=0)])
    col = np.concatenate([col, col[:300], col[:300], np.repeat(col[5:6], 250, axis=0)])
    xo, co, mo = orc.sor_filter(xyz, col, mean_k=k, stddev_mul=0.5, z_limit=0.0)
    xs, cs, ms = sn.sor_filter(xyz, col, mean_k=k, stddev_mul=0.5, z_limit=0.0)
    assert np.array_equal(ms, mo) and np.array_equal(xs, xo) and np.array_equal(cs, co)


@pytest.mark.parametrize("n,k", [(1500, 200), (400, 20), (64, 8), (2, 200)])
def test_matches_dense_restatement(n, k):
    xyz, _ = cloud(n, seed=n + 3, outliers=n // 50)
    keep0, dist, keep = numpy_sor(xyz, k, 0.01, 500.0)
    xs, _, ms = sn.sor_filter(xyz, None, mean_k=k, stddev_mul=0.01, z_limit=500.0)
    assert np.array_equal(ms, dist)
    assert np.array_equal(xs, xyz[keep0][keep])


def test_kd_tree_candidates_equal_brute_force():
    rng = np.random.default_rng(2)
    p = rng.normal(0, 2, (5000, 3)).astype(np.float32)
    p[:2000] = np.round(p[:2000] * 4) / 4           # a lattice-like part: many exact ties
    for k in (1, 20, 256):
        assert np.array_equal(sn.mean_distances(p, k), sn._brute_rows(p, np.arange(len(p)), k))


def test_hand_cases():
    # a line: nearest other points at 1, 1, 2, 7; mean 2.75, stddev sqrt(8.25); 0.8 stddev keeps the first three
    xyz = np.array([[0, 0, 0], [1, 0, 0], [3, 0, 0], [10, 0, 0]], np.float32)
    x, c, d = sn.sor_filter(xyz, xyz + 1, mean_k=1, stddev_mul=0.8)
    assert d.tolist() == [1, 1, 2, 7]
    assert np.array_equal(x, xyz[:3]) and np.array_equal(c, xyz[:3] + 1)
    # mean_k above m - 1: every other point counts; (0: 1 + 3) / 2, (1: 1 + 2) / 2, (3: 3 + 2) / 2
    _, _, d = sn.sor_filter(xyz[:3], mean_k=20, stddev_mul=0.8)
    assert d.tolist() == [2.0, 1.5, 2.5]
    # one point: no neighbours, distance 0, kept; none: nothing
    x, _, d = sn.sor_filter(xyz[:1])
    assert d.tolist() == [0.0] and len(x) == 1
    x, c, d = sn.sor_filter(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32))
    assert len(x) == len(c) == len(d) == 0
    # identical points: every distance 0, all kept
    x, _, d = sn.sor_filter(np.ones((50, 3), np.float32), mean_k=20)
    assert not d.any() and len(x) == 50


def test_non_finite_and_z_prefilter():
    xyz = np.array([[0, 0, -1], [1, 0, -1], [np.nan, 0, -1], [2, 0, -1], [0, np.inf, -1], [3, 0, -700],
                    [4, 0, -1]], np.float32)
    assert sn.prefilter(xyz, 0.0).tolist() == [True, True, False, True, False, True, True]
    assert sn.prefilter(xyz, 500.0).tolist() == [True, True, False, True, False, False, True]
    x, _, d = sn.sor_filter(xyz, mean_k=1, stddev_mul=10.0, z_limit=500.0)
    assert d.tolist() == [1, 1, 1, 2]            # the NaN and infinite points are not neighbours of anyone
    assert np.array_equal(x, xyz[[0, 1, 3, 6]])
