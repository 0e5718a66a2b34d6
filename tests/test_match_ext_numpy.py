"""tests/match_ext_numpy.py against naive double loops, and the properties its docstring states (M1 ... M8): MUTUAL's symmetry, a
hand-made case where CV and MUTUAL differ, the radius' boundaries, the gate's boundaries, and proof that the fixtures reach the
branches they are named for (CPU only)."""
import numpy as np
import pytest

import match_ext_numpy as mx
import match_numpy as mn

NORMS = pytest.mark.parametrize("norm", [mn.L2_F32, mn.L2_U8, mn.HAMMING], ids=["l2_f32", "l2_u8", "hamming"])


def rows(rng, n, dim, norm, tied):
    if norm == mn.L2_F32:
        return rng.integers(-2, 3, (n, dim)).astype(np.float32) if tied else rng.normal(size=(n, dim)).astype(np.float32)
    if norm == mn.L2_U8:
        return rng.integers(0, 3 if tied else 256, (n, dim)).astype(np.uint8)
    return rng.integers(0, 4 if tied else 2**32, (n, dim), np.uint64).astype(np.uint32)


def fixtures(norm):
    rng = np.random.default_rng(40 + norm)
    dim = {mn.L2_F32: 5, mn.L2_U8: 8, mn.HAMMING: 2}[norm]
    for tied in (False, True):
        for nq, nt in ((0, 3), (3, 0), (1, 1), (7, 9), (12, 5), (20, 20)):
            q, t = rows(rng, nq, dim, norm, tied), rows(rng, nt, dim, norm, tied)
            if tied and nq > 2 and nt > 2:
                t[2], q[1] = t[0], q[0]
            yield q, t, mn.keys(q, t, norm), tied


def same(a, b):
    return all(np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True) and np.asarray(x).dtype == np.asarray(y).dtype for x, y in zip(a, b))


@NORMS
def test_restatement_equals_the_naive_loops(norm):
    rng = np.random.default_rng(norm)
    ties = 0
    for q, t, key, tied in fixtures(norm):
        nq, nt = key.shape
        for mode in (mx.MUTUAL, mx.CV):
            assert same(mx.cross_from_keys(key, norm, mode), mx.naive_cross(key, norm, mode))
        for r in (0.0, 1.0, 2.5, float(np.median(mx.root(key, norm))) if key.size else 3.0, np.inf):
            assert same(mx.radius_from_keys(key, norm, r), mx.naive_radius(key, norm, r))
        mask = (rng.random((nq, nt)) < 0.4).astype(np.uint8)
        for k in (1, 2, 4):
            assert same(mx.masked_from_keys(key, mask, k, norm), mx.naive_masked(key, mask, k, norm))
            assert same(mx.masked_from_keys(key, np.ones((nq, nt)), k, norm), mn.select(key, k, norm))      # all pass: knn_match
        xq, xt = (rng.integers(0, 12, (nq, 2)) * 0.5).astype(np.float32), (rng.integers(0, 12, (nt, 2)) * 0.5).astype(np.float32)
        assert np.array_equal(mx.gate_mask(xq, xt, (1.0, 0.0, 2.5)), mx.naive_gate(xq, xt, (1.0, 0.0, 2.5)))
        if tied and key.size:
            ties += int((np.sort(key, axis=1)[:, :-1] == np.sort(key, axis=1)[:, 1:]).sum())
    assert ties > 10, "the tied fixtures hold no tie"


@NORMS
def test_mutual_is_symmetric_and_cv_keeps_its_pairs(norm):
    extra = 0
    for q, t, key, tied in fixtures(norm):
        fi, fd = mx.cross_from_keys(key, norm, mx.MUTUAL)
        ri, rd = mx.cross_from_keys(np.ascontiguousarray(key.T), norm, mx.MUTUAL)      # query and train swapped
        pairs = {(i, int(j)) for i, j in enumerate(fi) if j >= 0}
        assert pairs == {(int(i), j) for j, i in enumerate(ri) if i >= 0}
        for i, j in pairs:
            assert fd[i].tobytes() == rd[j].tobytes()
        ci, _ = mx.cross_from_keys(key, norm, mx.CV)
        assert all(ci[i] == j for i, j in pairs)                                          # M5
        extra += int(np.sum((ci >= 0) & (fi < 0)))
    assert extra > 0


def test_a_hand_made_case_where_cv_differs_from_mutual():
    """keys (query x train): query 0 is nearest to train 0, and train 0 to query 0 -- a mutual pair.  Train 1's best query is query
    1 (3 < 5), but query 1's own best is train 0 (2 < 3): MUTUAL leaves query 1 alone, CV pairs it with train 1."""
    key = np.array([[1, 5], [2, 3]], np.int64)
    mi, md = mx.cross_from_keys(key, mn.HAMMING, mx.MUTUAL)
    ci, cd = mx.cross_from_keys(key, mn.HAMMING, mx.CV)
    assert list(mi) == [0, -1] and list(md) == [1.0, np.inf]
    assert list(ci) == [0, 1] and list(cd) == [1.0, 3.0]
    # CV's strict < over ascending train rows: two train rows choose query 0 with one key, the lower one stays
    key = np.array([[4, 4, 9], [7, 7, 1]], np.int64)
    assert list(mx.cross_from_keys(key, mn.HAMMING, mx.CV)[0]) == [0, 2]
    assert list(mx.naive_cross(key, mn.HAMMING, mx.CV)[0]) == [0, 2]
    # comparisons on the key, not on the rooted float (M1): keys k and k + 1 with one root; the smaller KEY wins although the
    # larger one comes first
    k0 = next(k for k in range(16000001, 16000100) if np.sqrt(np.float32(k)) == np.sqrt(np.float32(k + 1)))
    key = np.array([[k0 + 1, k0]], np.int64)
    for mode in (mx.MUTUAL, mx.CV):
        assert list(mx.cross_from_keys(key, mn.L2_U8, mode)[0]) == [1]
    # a NaN key: behind every number; in CV it chooses nobody
    key = np.array([[np.nan, 2.0], [np.nan, np.nan]], np.float32)
    assert list(mx.cross_from_keys(key, mn.L2_F32, mx.MUTUAL)[0]) == [1, -1]
    assert list(mx.cross_from_keys(key, mn.L2_F32, mx.CV)[0]) == [1, -1]
    allnan = np.full((2, 2), np.nan, np.float32)
    assert list(mx.cross_from_keys(allnan, mn.L2_F32, mx.MUTUAL)[0]) == [0, -1] and list(mx.cross_from_keys(allnan, mn.L2_F32, mx.CV)[0]) == [-1, -1]


def test_radius_boundaries():
    r = np.float32(1.7320508)                             # sqrt(3) rounded
    below, above = np.nextafter(r, np.float32(0)), np.nextafter(r, np.float32(9))
    key = np.array([[3, 2, 4, 3]], np.int64)
    assert mx.root(key, mn.L2_U8)[0, 0] == r
    off, idx, dist = mx.radius_from_keys(key, mn.L2_U8, r)                     # dist == max_distance is kept
    assert list(off) == [0, 3] and list(idx) == [1, 0, 3] and dist[1] == r and dist[2] == r
    assert list(mx.radius_from_keys(key, mn.L2_U8, below)[1]) == [1]           # the next float below drops both
    assert list(mx.radius_from_keys(key, mn.L2_U8, above)[1]) == [1, 0, 3]
    # two different integer keys whose roots round to the same float: one radius takes both, in key order
    k0 = next(k for k in range(16000001, 16000100) if np.sqrt(np.float32(k)) == np.sqrt(np.float32(k + 1)))
    key = np.array([[k0 + 1, k0, k0 + 40]], np.int64)
    rr = np.sqrt(np.float32(k0))
    off, idx, dist = mx.radius_from_keys(key, mn.L2_U8, rr)
    assert list(idx) == [1, 0] and dist[0] == dist[1] == rr
    assert list(mx.radius_from_keys(key, mn.L2_U8, np.nextafter(rr, np.float32(0)))[0]) == [0, 0]
    # HAMMING compares the count as a float
    key = np.array([[3, 4, 2]], np.int64)
    assert list(mx.radius_from_keys(key, mn.HAMMING, 3.0)[1]) == [2, 0] and list(mx.radius_from_keys(key, mn.HAMMING, 2.999)[1]) == [2]
    # a NaN row never passes, not even an infinite radius; +inf does
    q = np.array([[0, 0], [np.nan, 0], [np.inf, 0]], np.float32)
    t = np.array([[1, 0], [0, np.nan], [3, 4]], np.float32)
    off, idx, dist = mx.radius_match(q, t, np.inf, mn.L2_F32)
    assert list(off) == [0, 2, 2, 4] and list(idx) == [0, 2, 0, 2] and np.isinf(dist[2:]).all() and not np.isnan(dist).any()
    assert list(mx.radius_match(q, t, -1.0, mn.L2_F32)[0]) == [0, 0, 0, 0]


def test_gate_boundaries():
    one = np.float32(1)
    up, down = np.nextafter(one, np.float32(2)), np.nextafter(one, np.float32(0))
    q = np.zeros((1, 2), np.float32)                      # at the origin: every difference below is exact
    # (x, y) of train rows: |dy| exactly dy_max and the next float beyond, on both sides; dx the float below dx_min, dx_min, dx_max
    # and the float above dx_max; a NaN in either coordinate
    t = np.array([[-1.5, 1], [-1.5, -1], [-1.5, up], [-1.5, -up], [-down, 0], [-one, 0], [-2 * one, 0],
                  [-np.nextafter(np.float32(2), np.float32(3)), 0], [np.nan, 0], [-1.5, np.nan]], np.float32)
    gate = (1.0, float(one), 2.0)
    dx = q[0, 0] - t[:, 0]
    assert dx[4] < one and dx[5] == one and dx[6] == 2 and dx[7] > 2
    assert list(mx.gate_mask(q, t, gate)[0]) == [1, 1, 0, 0, 0, 1, 1, 0, 0, 0]
    assert np.array_equal(mx.gate_mask(q, t, gate), mx.naive_gate(q, t, gate))
    assert not mx.gate_mask(q, t, (np.nan, 0.0, 2.0)).any()


def test_the_fixtures_reach_their_branches():
    rng = np.random.default_rng(8)
    q, t = rng.integers(0, 256, (4, 8)).astype(np.uint8), rng.integers(0, 256, (6, 8)).astype(np.uint8)
    mask = np.ones((4, 6), np.uint8)
    mask[0] = 0                      # a query with 0 candidates
    mask[1] = 0
    mask[1, 4] = 7                   # a query with 1 < k candidates
    idx, dist = mx.knn_match_masked(q, t, mask, 2, mn.L2_U8)
    assert list(idx[0]) == [-1, -1] and np.isinf(dist[0]).all()
    assert list(idx[1]) == [4, -1] and np.isfinite(dist[1, 0]) and np.isinf(dist[1, 1])
    assert (idx[2:] >= 0).all() and same((idx[2:], dist[2:]), tuple(a[2:] for a in mn.knn_match(q, t, 2, mn.L2_U8)))
    # a query past the per-query bound
    key = np.zeros((2, mx.MAX_PER_QUERY + 1), np.int64)
    key[1] = 9
    off = mx.radius_from_keys(key, mn.HAMMING, 0.0)[0]
    assert list(off) == [0, mx.MAX_PER_QUERY + 1, mx.MAX_PER_QUERY + 1] and mx.radius_verdict(off, 10**6) == "capacity"
    off = mx.radius_from_keys(key[:, :-1], mn.HAMMING, 0.0)[0]
    assert mx.radius_verdict(off, mx.MAX_PER_QUERY) == "ok" and mx.radius_verdict(off, mx.MAX_PER_QUERY - 1) == "capacity"
