"""tests/match_numpy.py -- the restatement of svo_knn_match / svo_ratio_pairs -- against naive per-pair loops and against
the properties include/svo.h states (CPU only)."""
import numpy as np
import pytest

import match_numpy as mn


def _same(a, b):
    assert np.array_equal(a[0], b[0])
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


@pytest.mark.parametrize("norm", [mn.L2_F32, mn.L2_U8, mn.HAMMING])
@pytest.mark.parametrize("k", [1, 2, 4])
def test_vectorised_equals_the_naive_loop(norm, k):
    rng = np.random.default_rng(10 * norm + k)
    for nq, nt, dim in [(1, 1, 1 if norm != mn.L2_U8 else 4), (5, 7, 8), (9, 3, 16), (13, 17, 12)]:
        if norm == mn.L2_F32:
            q, t = rng.normal(size=(nq, dim)).astype(np.float32), rng.normal(size=(nt, dim)).astype(np.float32)
        elif norm == mn.L2_U8:
            q, t = rng.integers(0, 256, (nq, dim), np.uint8), rng.integers(0, 256, (nt, dim), np.uint8)
        else:
            q = rng.integers(0, 2**32, (nq, dim), np.uint64).astype(np.uint32)
            t = rng.integers(0, 2**32, (nt, dim), np.uint64).astype(np.uint32)
        _same(mn.knn_match(q, t, k, norm), mn.naive_knn(q, t, k, norm))


def test_float_key_is_the_stated_sum_not_a_dot_product():
    # squares 1, 2^-24, 2^-24: the stated sequence s = s + t*t rounds 1 + 2^-24 back to 1 twice (ties to even); the exact
    # sum 1 + 2^-23 is a float of its own -- any other order or a wider accumulator gives that one
    q = np.array([[1.0, 2.0**-12, 2.0**-12]], np.float32)
    t = np.zeros((1, 3), np.float32)
    assert mn.keys(q, t, mn.L2_F32)[0, 0] == np.float32(1)
    assert mn.keys(q[:, ::-1], t, mn.L2_F32)[0, 0] == np.float32(1 + 2.0**-23)
    assert np.float32(np.sum(q[0].astype(np.float64) ** 2)) == np.float32(1 + 2.0**-23)
    assert mn.naive_key(q[0], t[0], mn.L2_F32) == np.float32(1)


@pytest.mark.parametrize("dim", [32, 256])
def test_bytes_give_the_bits_of_the_converted_floats(dim):
    rng = np.random.default_rng(dim)
    q, t = rng.integers(0, 256, (40, dim), np.uint8), rng.integers(0, 256, (50, dim), np.uint8)
    q[0], t[0], t[1] = 0, 255, 0        # the largest possible sum: dim * 255^2 < 2^24
    q[1], t[2] = 255, 0
    assert dim * 255 * 255 < 2**24
    for k in (1, 2, 4):
        _same(mn.knn_match(q, t, k, mn.L2_U8), mn.knn_match(q.astype(np.float32), t.astype(np.float32), k, mn.L2_F32))
    idx, dist = mn.knn_match(q, t, 2, mn.L2_U8)
    assert idx[0, 0] == 1 and dist[0, 0] == 0
    k_u8 = mn.keys(q[:2], t[:3], mn.L2_U8)
    assert k_u8[0, 0] == dim * 255 * 255 and k_u8[1, 2] == dim * 255 * 255
    # any summation order: the reversed float sum has the same bits
    rev = mn.keys(q[:, ::-1].astype(np.float32), t[:, ::-1].astype(np.float32), mn.L2_F32)
    assert np.array_equal(rev, mn.keys(q.astype(np.float32), t.astype(np.float32), mn.L2_F32))


@pytest.mark.parametrize("norm", [mn.L2_F32, mn.L2_U8, mn.HAMMING])
def test_duplicated_train_rows_resolve_to_the_lower_index(norm):
    rng = np.random.default_rng(norm)
    if norm == mn.L2_F32:
        q, t = rng.normal(size=(6, 8)).astype(np.float32), rng.normal(size=(12, 8)).astype(np.float32)
    elif norm == mn.L2_U8:
        q, t = rng.integers(0, 256, (6, 8), np.uint8), rng.integers(0, 256, (12, 8), np.uint8)
    else:
        q = rng.integers(0, 2**32, (6, 8), np.uint64).astype(np.uint32)
        t = rng.integers(0, 2**32, (12, 8), np.uint64).astype(np.uint32)
    t[9], t[4], t[2] = q[0], q[0], q[0]          # an exact three-way tie at distance zero
    idx, dist = mn.knn_match(q, t, 4, norm)
    assert list(idx[0, :3]) == [2, 4, 9] and np.all(dist[0, :3] == 0)
    t[:] = t[0]                                   # every row alike: index order
    idx, _ = mn.knn_match(q, t, 4, norm)
    assert np.array_equal(idx, np.tile(np.arange(4, dtype=np.int32), (6, 1)))


def test_fewer_train_rows_than_k_leave_empty_slots():
    q = np.arange(12, dtype=np.float32).reshape(3, 4)
    idx, dist = mn.knn_match(q, q[:1], 4, mn.L2_F32)
    assert np.array_equal(idx[:, 0], [0, 0, 0]) and np.all(idx[:, 1:] == -1)
    assert np.all(np.isinf(dist[:, 1:])) and np.all(dist[:, 1:] > 0) and np.all(np.isfinite(dist[:, 0]))
    idx, dist = mn.knn_match(q, q[:0], 2, mn.L2_F32)
    assert np.all(idx == -1) and np.all(np.isinf(dist))
    idx, dist = mn.knn_match(q[:0], q, 2, mn.L2_F32)
    assert idx.shape == (0, 2) and dist.shape == (0, 2)


def test_ratio_pairs_drops_a_query_whose_second_slot_is_empty():
    idx = np.array([[0, -1], [1, 0], [0, 1]], np.int32)
    dist = np.array([[0.0, np.inf], [1.0, 2.0], [3.0, 3.5]], np.float32)
    xq = np.array([[10, 11], [20, 21], [30, 31]], np.float32)
    xt = np.array([[1, 2], [3, 4]], np.float32)
    p1, p2, mask = mn.ratio_pairs(idx, dist, xq, xt, 0.8)
    assert list(mask) == [0, 1, 0]                # 0 < 0.8 * inf would hold: the empty slot drops the query
    assert np.array_equal(p1, [[20, 21]]) and np.array_equal(p2, [[3, 4]])
    p1, p2, mask = mn.ratio_pairs(idx[:, :1], dist[:, :1], xq, xt, 0.8)
    assert not mask.any() and len(p1) == 0 and len(p2) == 0   # k = 1: no second neighbour to compare with


def test_ratio_comparison_is_made_in_double():
    # 0.8 as a double is 0.8000000000000000444: 0.8 * 5 rounds to exactly 4.0 in double, so 4 < 0.8 * 5 is false -- as in
    # the C++ expression m.distance < 0.8 * n.distance, whose float operands are promoted to double.
    assert not (4.0 < 0.8 * 5.0)
    idx = np.array([[0, 1], [0, 1], [0, 1]], np.int32)
    below = np.nextafter(np.float32(4), np.float32(0))
    dist = np.array([[4, 5], [below, 5], [4, np.nextafter(np.float32(5), np.float32(6))]], np.float32)
    xy = np.zeros((3, 2), np.float32)
    _, _, mask = mn.ratio_pairs(idx, dist, xy, xy, 0.8)
    assert list(mask) == [0, 1, 1]
    _, _, mask = mn.ratio_pairs(idx, dist, xy, xy, 1.0)
    assert list(mask) == [1, 1, 1]


def test_batch_is_the_problems_one_by_one():
    rng = np.random.default_rng(5)
    q, t = rng.integers(0, 256, (20, 8), np.uint8), rng.integers(0, 256, (15, 8), np.uint8)
    qo, to = [0, 7, 7, 20], [0, 1, 6, 15]
    idx, dist = mn.knn_match_batch(q, t, qo, to, 2, mn.L2_U8)
    assert np.all(idx[:7, 1] == -1) and np.all(idx[:7, 0] == 0)
    i2, d2 = mn.knn_match(q[7:], t[6:], 2, mn.L2_U8)
    assert np.array_equal(idx[7:], i2) and np.array_equal(dist[7:], d2)
