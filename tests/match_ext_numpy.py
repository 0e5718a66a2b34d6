"""cv::BFMatcher's cross-check, radiusMatch and masked knnMatch restated in numpy exactly as include/svo.h specifies
svo_match_cross / svo_radius_match / svo_knn_match_gated, on top of the keys and the selection of tests/match_numpy.py.  Test
infrastructure: nothing here imports the library, and every function forms the full nq x nt key matrix the library never forms.

The points of the restatement, each RECALLED (how OpenCV 3.2 behaves, from memory: no OpenCV can run here) or OURS (decided here
and kept fixed):

M1  OURS      Every comparison is made on the SELECTION KEY (match_numpy.keys), never on the rooted float.  Two integer keys whose
              roots round to the same float still order by key.  The one exception is M6, which the issue words otherwise.
M2  OURS      The order everywhere: ascending key, equal keys to the lower index, a NaN key behind every number (+inf included).
M3  OURS      CROSS_MUTUAL: query i is paired with train j exactly when j is first among the train rows for i and i is first among
              the query rows for j, both by M2.  A NaN key takes part like any key (an all-NaN row's first partner is index 0).
M4  RECALLED  CROSS_CV, batchDistance(src1, src2, ..., crosscheck = true): only the reverse search batchDistance(src2, src1, K = 1)
              runs; dist starts at the type's maximum and nidx at -1; then `for i in train rows ascending: idx = tidx[i]; d = tdist[i];
              if (d < dist[idx]) { dist[idx] = d; nidx[idx] = i; }`.  The strict < keeps the lower train row on a tie, and a NaN d
              updates nothing.  OURS: d is compared as a key (M1); the reverse search follows M2 (OpenCV's own tie rule inside
              batchDistance is not recalled); a query nobody chose gets -1 / +inf (OpenCV drops it from the match list).
M5  OURS      Consequence of M3 / M4, checked in tests/test_match_ext_numpy.py: without NaN keys every MUTUAL pair is a CV pair,
              and CV can pair a query whose own best train row is another one.
M6  RECALLED  radiusMatch keeps a train row when dist <= maxDistance, on the FLOAT that is returned (rooted for the L2 norms, the
              count for HAMMING); a NaN dist never passes.  OURS: each query's matches in the order M2 (on keys: among keys with
              one rooted float the smaller key is first); CSR output; the per-query bound MAX_PER_QUERY and the capacity refusal.
M7  RECALLED  knnMatch with a mask: a pair whose mask byte is zero does not exist for the search; a query with fewer than k
              allowed rows has fewer matches.  OURS: the missing slots are -1 / +inf, as svo_knn_match's.
M8  OURS      The geometric gate: train row t is a candidate of query q when fabsf(y_q - y_t) <= dy_max and dx_min <= x_q - x_t <=
              dx_max, each a float32 operation of its own in that order; a NaN anywhere fails.
"""
import numpy as np

from match_numpy import HAMMING, L2_F32, L2_U8, keys, select  # noqa: F401

MUTUAL, CV = 0, 1
MAX_PER_QUERY = 8192     # SVO_RADIUS_MAX_PER_QUERY


def sort_key(key):
    """a key matrix as float64 with NaN -> +inf's successor, so that a stable argsort is the order M2"""
    k = np.asarray(key, np.float64).copy()
    with np.errstate(invalid="ignore"):
        k[np.isinf(k)] = np.finfo(np.float64).max    # float keys are float32: nothing real is this large
    k[np.isnan(k)] = np.inf
    return k


def root(key, norm):
    """the returned float of a key (array)"""
    key = np.asarray(key)
    if norm == HAMMING:
        return key.astype(np.float32)
    with np.errstate(invalid="ignore"):
        return np.sqrt(key.astype(np.float32))


def first(key, axis):
    """index of the first element by M2 along an axis (-1 where the axis is empty)"""
    if key.shape[axis] == 0:
        return np.full(key.shape[1 - axis], -1, np.int64)
    return np.argsort(sort_key(key), axis=axis, kind="stable").take(0, axis=axis)


def cross_from_keys(key, norm, mode):
    nq, nt = key.shape
    idx, dist = np.full(nq, -1, np.int32), np.full(nq, np.inf, np.float32)
    if nq == 0 or nt == 0:
        return idx, dist
    best_q = first(key, 0)                      # per train row: its query
    if mode == MUTUAL:
        best_t = first(key, 1)
        for i in range(nq):
            j = int(best_t[i])
            if int(best_q[j]) == i:
                idx[i], dist[i] = j, root(key[i, j], norm)
        return idx, dist
    held = [None] * nq                          # the key a query holds
    for j in range(nt):                         # ascending train rows, strict <
        i = int(best_q[j])
        d = key[i, j]
        if d != d:
            continue
        if held[i] is None or d < held[i]:
            held[i], idx[i] = d, j
    for i in range(nq):
        if held[i] is not None:
            dist[i] = root(held[i], norm)
    return idx, dist


def match_cross(query, train, norm=L2_U8, mode=MUTUAL):
    return cross_from_keys(keys(np.asarray(query), np.asarray(train), norm), norm, mode)


def radius_from_keys(key, norm, max_distance):
    """-> (row_offsets [nq + 1] int64, idx int32, dist float32); the caller applies capacity and MAX_PER_QUERY"""
    nq, nt = key.shape
    r = np.float32(max_distance)
    d = root(key, norm).reshape(nq, nt)
    with np.errstate(invalid="ignore"):
        keep = d <= r                           # a NaN is False
    sk = sort_key(key)
    off, idx, dist = [0], [], []
    for i in range(nq):
        c = np.flatnonzero(keep[i])
        c = c[np.argsort(sk[i, c], kind="stable")]
        idx.append(c)
        dist.append(d[i, c])
        off.append(off[-1] + len(c))
    cat = lambda parts, t: np.concatenate(parts).astype(t) if parts else np.zeros(0, t)
    return np.array(off, np.int64), cat(idx, np.int32), cat(dist, np.float32)


def radius_match(query, train, max_distance, norm=L2_U8):
    return radius_from_keys(keys(np.asarray(query), np.asarray(train), norm), norm, max_distance)


def radius_verdict(row_offsets, capacity):
    """what svo_radius_match returns for these offsets: 'ok', or 'capacity' (the total or one row too large)"""
    counts = np.diff(row_offsets)
    return "ok" if row_offsets[-1] <= capacity and (len(counts) == 0 or counts.max() <= MAX_PER_QUERY) else "capacity"


def gate_mask(xy_query, xy_train, gate):
    """M8 as an nq x nt byte matrix"""
    xq, xt = np.asarray(xy_query, np.float32).reshape(-1, 2), np.asarray(xy_train, np.float32).reshape(-1, 2)
    dy_max, dx_min, dx_max = (np.float32(v) for v in gate)
    with np.errstate(invalid="ignore", over="ignore"):
        ady = np.abs(xq[:, None, 1] - xt[None, :, 1])          # float32 throughout
        dx = xq[:, None, 0] - xt[None, :, 0]
        return ((ady <= dy_max) & (dx >= dx_min) & (dx <= dx_max)).astype(np.uint8)


def masked_from_keys(key, mask, k, norm):
    nq, nt = key.shape
    mask = np.asarray(mask).reshape(nq, nt) != 0
    idx, dist = np.full((nq, k), -1, np.int32), np.full((nq, k), np.inf, np.float32)
    sk = sort_key(key)
    for i in range(nq):
        c = np.flatnonzero(mask[i])
        c = c[np.argsort(sk[i, c], kind="stable")][:k]
        idx[i, :len(c)] = c
        dist[i, :len(c)] = root(key[i, c], norm)
    return idx, dist


def knn_match_masked(query, train, mask, k=2, norm=L2_U8):
    return masked_from_keys(keys(np.asarray(query), np.asarray(train), norm), mask, k, norm)


def knn_match_gated(query, train, xy_query, xy_train, gate, k=2, norm=L2_U8):
    return knn_match_masked(query, train, gate_mask(xy_query, xy_train, gate), k, norm)


def batch(fn, query, train, q_offsets, t_offsets):
    """fn(query rows, train rows, p) per problem -> list of results"""
    return [fn(query[int(q_offsets[p]):int(q_offsets[p + 1])], train[int(t_offsets[p]):int(t_offsets[p + 1])], p)
            for p in range(len(q_offsets) - 1)]


# ---- naive double loops (tests/test_match_ext_numpy.py checks the forms above against these) ------------------------
def _before(a, b):
    """(key, index) a orders before b by M2"""
    (ka, ia), (kb, ib) = a, b
    na, nb = ka != ka, kb != kb
    if na != nb:
        return nb
    if na or ka == kb:
        return ia < ib
    return ka < kb


def naive_first(cands):
    best = None
    for c in cands:
        if best is None or _before(c, best):
            best = c
    return best


def naive_cross(key, norm, mode):
    nq, nt = key.shape
    idx, dist = np.full(nq, -1, np.int32), np.full(nq, np.inf, np.float32)
    if nq == 0 or nt == 0:
        return idx, dist
    q_of = [naive_first([(key[i, j], i) for i in range(nq)])[1] for j in range(nt)]
    if mode == MUTUAL:
        for i in range(nq):
            j = naive_first([(key[i, j], j) for j in range(nt)])[1]
            if q_of[j] == i:
                idx[i], dist[i] = j, root(key[i, j], norm)
        return idx, dist
    d0 = [None] * nq
    for j in range(nt):
        i, d = q_of[j], key[q_of[j], j]
        if d == d and (d0[i] is None or d < d0[i]):
            d0[i], idx[i], dist[i] = d, j, root(d, norm)
    return idx, dist


def naive_sorted(cands):
    out = []
    for c in cands:                         # insertion by M2
        p = len(out)
        while p > 0 and _before(c, out[p - 1]):
            p -= 1
        out.insert(p, c)
    return out


def naive_radius(key, norm, max_distance):
    r = np.float32(max_distance)
    off, idx, dist = [0], [], []
    for i in range(key.shape[0]):
        row = naive_sorted([(key[i, j], j) for j in range(key.shape[1]) if root(key[i, j], norm) <= r])
        idx += [j for _, j in row]
        dist += [root(kk, norm) for kk, _ in row]
        off.append(len(idx))
    return np.array(off, np.int64), np.array(idx, np.int32), np.array(dist, np.float32)


def naive_masked(key, mask, k, norm):
    nq, nt = key.shape
    idx, dist = np.full((nq, k), -1, np.int32), np.full((nq, k), np.inf, np.float32)
    for i in range(nq):
        row = naive_sorted([(key[i, j], j) for j in range(nt) if mask[i][j]])[:k]
        for s, (kk, j) in enumerate(row):
            idx[i, s], dist[i, s] = j, root(kk, norm)
    return idx, dist


def naive_gate(xq, xt, gate):
    dy_max, dx_min, dx_max = (np.float32(v) for v in gate)
    out = np.zeros((len(xq), len(xt)), np.uint8)
    for i, (x1, y1) in enumerate(np.asarray(xq, np.float32).reshape(-1, 2)):
        for j, (x2, y2) in enumerate(np.asarray(xt, np.float32).reshape(-1, 2)):
            ady = np.float32(abs(np.float32(y1 - y2)))
            dx = np.float32(x1 - x2)
            out[i, j] = 1 if (ady <= dy_max and dx >= dx_min and dx <= dx_max) else 0
    return out
