"""cv::BFMatcher(normType, false).knnMatch and the ratio-test loop of src/triangulation.cpp:123-133, restated in numpy
exactly as include/svo.h specifies svo_knn_match / svo_ratio_pairs.  Test infrastructure: nothing here imports the
library.

Selection key per (query, train) pair:
  L2_F32   s = 0; for i in 0..dim-1: t = a_i - b_i; s = s + t*t   -- float32, every operation rounded on its own, one
           accumulator, index order (numpy's float32 array arithmetic rounds each operation; there is no FMA)
  L2_U8    the exact integer sum of (a_i - b_i)^2
  HAMMING  popcount of the xor of the uint32 words
Order: ascending key, equal keys to the lower train index (a stable argsort); NaN keys after every number.
dist: float32 sqrt of the key (correctly rounded) for the two L2 norms, the count as a float for HAMMING.
Fewer than k train rows: idx -1, dist +inf.
"""
import numpy as np

L2_F32, L2_U8, HAMMING = 0, 1, 2

_POP8 = np.array([bin(i).count("1") for i in range(256)], np.uint8)


def keys(query, train, norm, chunk=512):
    """nq x nt keys: float32 for L2_F32, int64 for L2_U8 and HAMMING."""
    if norm == L2_F32:
        q, t = np.ascontiguousarray(query, np.float32), np.ascontiguousarray(train, np.float32)
        out = np.zeros((q.shape[0], t.shape[0]), np.float32)
        for r0 in range(0, q.shape[0], chunk):
            s = out[r0:r0 + chunk]
            for i in range(q.shape[1]):
                d = q[r0:r0 + chunk, i, None] - t[None, :, i]   # float32 - float32 -> float32, rounded once
                d *= d
                s += d
        return out
    if norm == L2_U8:
        q, t = np.ascontiguousarray(query, np.uint8).astype(np.int64), np.ascontiguousarray(train, np.uint8).astype(np.int64)
        out = np.zeros((q.shape[0], t.shape[0]), np.int64)
        for r0 in range(0, q.shape[0], chunk):
            for i in range(q.shape[1]):
                d = q[r0:r0 + chunk, i, None] - t[None, :, i]
                out[r0:r0 + chunk] += d * d
        return out
    if norm == HAMMING:
        q, t = np.ascontiguousarray(query, np.uint32), np.ascontiguousarray(train, np.uint32)
        q, t = q.view(np.uint8).reshape(len(q), 4 * q.shape[1]), t.view(np.uint8).reshape(len(t), 4 * t.shape[1])
        out = np.zeros((q.shape[0], t.shape[0]), np.int64)
        for i in range(q.shape[1]):
            out += _POP8[q[:, i, None] ^ t[None, :, i]]
        return out
    raise ValueError(f"unknown norm {norm}")


def select(key, k, norm):
    """(idx [nq, k] int32, dist [nq, k] float32) of a key matrix."""
    nq, nt = key.shape
    idx = np.full((nq, k), -1, np.int32)
    dist = np.full((nq, k), np.inf, np.float32)
    m = min(k, nt)
    if nq == 0 or m == 0:
        return idx, dist
    order = np.argsort(key, axis=1, kind="stable")[:, :m]
    best = np.take_along_axis(key, order, axis=1)
    idx[:, :m] = order
    if norm == HAMMING:
        dist[:, :m] = best.astype(np.float32)
    else:
        # float32 sqrt of a float32 is correctly rounded; the integer keys are below 2^24, so exact as float32
        with np.errstate(invalid="ignore"):
            dist[:, :m] = np.sqrt(best.astype(np.float32))
    return idx, dist


def knn_match(query, train, k=2, norm=L2_U8):
    query, train = np.asarray(query), np.asarray(train)
    return select(keys(query, train, norm), k, norm)


def knn_match_batch(query, train, q_offsets, t_offsets, k=2, norm=L2_U8):
    """The batched call: problem p is query rows q_offsets[p]..q_offsets[p+1]-1 against train rows t_offsets[p]..; rows of
    idx / dist are the query rows, train indices local to the problem."""
    nq = int(q_offsets[-1])
    idx = np.full((nq, k), -1, np.int32)
    dist = np.full((nq, k), np.inf, np.float32)
    for p in range(len(q_offsets) - 1):
        a, b = int(q_offsets[p]), int(q_offsets[p + 1])
        i, d = knn_match(query[a:b], train[int(t_offsets[p]):int(t_offsets[p + 1])], k, norm)
        idx[a:b], dist[a:b] = i, d
    return idx, dist


def ratio_pairs(idx, dist, xy_query, xy_train, ratio=0.8):
    """if (m.distance < ratio * n.distance) of src/triangulation.cpp:129 -- float distances promoted to double, the product
    and the comparison in double -> (p1, p2, mask)."""
    idx = np.asarray(idx, np.int32)
    dist = np.asarray(dist, np.float32)
    nq, k = idx.shape
    xq = np.asarray(xy_query, np.float32).reshape(-1, 2)
    xt = np.asarray(xy_train, np.float32).reshape(-1, 2)
    mask = np.zeros(nq, np.uint8)
    if k >= 2 and nq > 0:
        with np.errstate(invalid="ignore"):
            keep = (idx[:, 1] >= 0) & (dist[:, 0].astype(np.float64) < np.float64(ratio) * dist[:, 1].astype(np.float64))
        mask[:] = keep
    sel = np.flatnonzero(mask)
    return xq[sel].copy(), xt[idx[sel, 0]].copy() if len(sel) else np.zeros((0, 2), np.float32), mask


# ---- naive per-pair loops (tests/test_match_numpy.py checks the vectorised forms against these) ----------------------
def naive_key(a, b, norm):
    if norm == L2_F32:
        s = np.float32(0)
        for x, y in zip(np.asarray(a, np.float32), np.asarray(b, np.float32)):
            t = np.float32(x - y)
            s = np.float32(s + np.float32(t * t))
        return s
    if norm == L2_U8:
        return sum((int(x) - int(y)) ** 2 for x, y in zip(a, b))
    return sum(bin(int(x) ^ int(y)).count("1") for x, y in zip(a, b))


def naive_knn(query, train, k, norm):
    idx = np.full((len(query), k), -1, np.int32)
    dist = np.full((len(query), k), np.inf, np.float32)
    for i, a in enumerate(query):
        cand = [(naive_key(a, b, norm), j) for j, b in enumerate(train)]
        cand.sort(key=lambda c: (c[0], c[1]))      # ascending key, then ascending train index
        for s, (key, j) in enumerate(cand[:k]):
            idx[i, s] = j
            dist[i, s] = np.float32(key) if norm == HAMMING else np.sqrt(np.float32(key))
    return idx, dist
