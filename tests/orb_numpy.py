"""A blind numpy restatement of the extractor in cv::ORB's shape, the third party beside the HIP kernels
(csrc/orb_cv.hip) and the C oracle (oracle/orb.c: orc_orb_extract_cv).

TEST INFRASTRUCTURE.  Written from the recipe in oracle/orb.c's header ("cv::ORB's own shape"), the FAST paper (Rosten &
Drummond 2006: a segment of nine contiguous ring pixels all brighter or all darker than the centre by more than t) and the ORB
paper (Rublee et al. 2011: intensity centroid, steered BRIEF), NOT from the kernel and not loop by loop from the oracle: whole
images at a time, arcs by their definition, convolutions through scipy.ndimage.correlate, selection through np.lexsort,
cos / sin through long double.  Every float32 operation is rounded on its own (numpy never fuses a multiply with an add).

orb_extract_cv(img, ...) -> (xy, octave, response, dir, angle, desc), levels
levels is the per-level record the edge-case tests use to prove which branch of the selection an image reaches.
"""
import numpy as np
from scipy import ndimage

F = np.float32
EDGE = 31                      # edgeThreshold
HALF_PATCH = 15                # patchSize 31
UMAX_TABLE = (15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3)

# the Bresenham circle of radius 3, clockwise from twelve o'clock: (dx, dy)
RING = ((0, -3), (1, -3), (2, -2), (3, -1), (3, 0), (3, 1), (2, 2), (1, 3),
        (0, 3), (-1, 3), (-2, 2), (-3, 1), (-3, 0), (-3, -1), (-2, -2), (-1, -3))


# ---------------------------------------------------------------------------------------------------- grey, levels, quota
def to_gray(img):
    """OpenCV's fixed-point BGR2GRAY; a single channel passes through."""
    img = np.asarray(img, np.uint8)
    if img.ndim == 2 or img.shape[2] == 1:
        return img.reshape(img.shape[0], img.shape[1]).copy()
    i = img.astype(np.int64)
    return ((1868 * i[..., 0] + 9617 * i[..., 1] + 4899 * i[..., 2] + 8192) >> 14).astype(np.uint8)


def levels_and_quota(w, h, n_levels, scale_factor, n_features):
    """-> (ws, hs, scales float32, quota): level l has scale (float)pow(sf, l) and size round(cols / scale); the quota is
    n (1 - f) / (1 - f^L) scaled by f = 1 / sf per level and rounded, the last level takes what is left (never below 0)."""
    sf = F(scale_factor)
    scales = np.array([F(float(sf) ** l) for l in range(n_levels)], F)
    ws = np.rint(F(w) / scales).astype(np.int64)
    hs = np.rint(F(h) / scales).astype(np.int64)
    f = F(1.0 / float(sf))
    want = F(F(n_features) * F(F(1) - f)) / F(F(1) - F(float(f) ** n_levels))
    quota = []
    for _ in range(n_levels - 1):
        quota.append(int(np.rint(want)))
        want = F(want * f)
    quota.append(max(n_features - sum(quota), 0))
    return ws, hs, scales, np.array(quota, np.int64)


# ---------------------------------------------------------------------------------------------------- resize, blur
def _resize_axis(src_len, dst_len):
    """Source index and the two 11-bit weights of each destination sample, at pixel centres."""
    scale = 1.0 / (float(dst_len) / float(src_len))
    f = ((np.arange(dst_len) + 0.5) * scale - 0.5).astype(F)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(F)).astype(F)
    return s, f


def resize_linear(src, dw, dh):
    """cv::resize(INTER_LINEAR) of one 8-bit channel: bilinear at pixel centres, coefficients round(2048 (1 - f)),
    round(2048 f) made in float32, integer products, upstream's 8-bit vertical pass (the horizontal sums lose 4 bits, each
    row product 16, then one rounding by 4)."""
    src = np.asarray(src, np.uint8)
    sh, sw = src.shape
    sx, fx = _resize_axis(sw, dw)
    # columns: a sample left of the first or at / right of the last source pixel IS that pixel
    out_l, out_r = sx < 0, sx >= sw - 1
    fx = np.where(out_l | out_r, F(0), fx)
    sx = np.where(out_l, 0, np.where(out_r, sw - 1, sx))
    a0 = np.rint((F(1) - fx) * F(2048)).astype(np.int64)
    a1 = np.rint(fx * F(2048)).astype(np.int64)
    s = src.astype(np.int64)
    rows = s[:, sx] * a0 + s[:, np.minimum(sx + 1, sw - 1)] * a1              # [sh, dw], 19 bits
    # rows: the weights keep their fraction, the two row indices are clamped into the image
    sy, fy = _resize_axis(sh, dh)
    b0 = np.rint((F(1) - fy) * F(2048)).astype(np.int64)[:, None]
    b1 = np.rint(fy * F(2048)).astype(np.int64)[:, None]
    r0, r1 = rows[np.clip(sy, 0, sh - 1)] >> 4, rows[np.clip(sy + 1, 0, sh - 1)] >> 4
    out = (((b0 * r0) >> 16) + ((b1 * r1) >> 16) + 2) >> 2
    return out.astype(np.uint8)


def gauss_kernel7():
    x = np.arange(-3, 4, dtype=np.float64)
    k = np.exp(-x * x / 8.0)                      # sigma 2
    return np.rint(k / k.sum() * 256).astype(np.int64)


def gauss7(g):
    """GaussianBlur 7x7, sigma 2, in 8-bit fixed point: exact integer sums, + 2^15 >> 16, saturated."""
    k = gauss_kernel7()
    s = ndimage.correlate(np.asarray(g).astype(np.int64), np.outer(k, k), mode="mirror")      # mirror = reflect-101
    return np.minimum((s + (1 << 15)) >> 16, 255).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------- FAST-9
def has_arc9(flags):
    """flags [..., 16] bool around the ring -> True where nine contiguous (cyclically) are set.  The definition: some
    start s with flags[s], flags[s + 1], ... flags[s + 8] all set, indices modulo 16."""
    flags = np.asarray(flags, bool)
    idx = (np.arange(16)[:, None] + np.arange(9)[None, :]) % 16                 # [start, member]
    return flags[..., idx].all(axis=-1).any(axis=-1)


def ring_differences(g):
    """-> int16 [16, h - 6, w - 6]: ring pixel minus centre for every pixel at least 3 inside."""
    g = np.asarray(g).astype(np.int16)
    h, w = g.shape
    c = g[3:h - 3, 3:w - 3]
    return np.stack([g[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] - c for dx, dy in RING])


def fast_fires_at(g, xs, ys, t):
    """The segment test at threshold t at the pixels (xs, ys), each at least 3 inside -> bool [n]."""
    g = np.asarray(g).astype(np.int16)
    d = np.stack([g[ys + dy, xs + dx] for dx, dy in RING], axis=-1) - g[ys, xs][..., None]
    return has_arc9(d > t) | has_arc9(d < -t)


def fast_fires(g, t):
    """The segment test at threshold t over the whole image -> bool [h, w] (False on the 3-pixel border)."""
    h, w = np.asarray(g).shape
    ys, xs = np.mgrid[3:h - 3, 3:w - 3]
    out = np.zeros((h, w), bool)
    out[3:-3, 3:-3] = fast_fires_at(g, xs, ys, t)
    return out


def fast_score_image(g, t):
    """cornerScore over the whole image -> uint8 [h, w]: the best over the 16 arcs of nine ring pixels of min(ring - centre)
    and of min(centre - ring), minus one; 0 where that falls below t (no corner at t) and on the 3-pixel border."""
    d = ring_differences(g)
    best = np.full(d.shape[1:], -256, np.int16)
    for s in range(16):
        arc = d[[(s + j) % 16 for j in range(9)]]
        best = np.maximum(best, np.maximum(arc.min(axis=0), (-arc).min(axis=0)))
    score = best - 1
    out = np.zeros(np.asarray(g).shape, np.uint8)
    out[3:-3, 3:-3] = np.where(score >= t, score, 0)
    return out


def suppress(score):
    """bool [h, w]: a non-zero score strictly above all eight neighbours, inside the 31-pixel margin."""
    h, w = score.shape
    keep = np.zeros((h, w), bool)
    if h <= 2 * EDGE or w <= 2 * EDGE:
        return keep
    s = score.astype(np.int16)
    c = s[EDGE:h - EDGE, EDGE:w - EDGE]
    ok = c > 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                ok &= c > s[EDGE + dy:h - EDGE + dy, EDGE + dx:w - EDGE + dx]
    keep[EDGE:h - EDGE, EDGE:w - EDGE] = ok
    return keep


# ---------------------------------------------------------------------------------------------------- Harris
def harris_image(g):
    """Harris response (7x7 block, k 0.04, Sobel-3 gradients as integer sums, the float32 formula) -> float32 [h, w];
    meaningful at least 4 pixels inside."""
    gi = np.asarray(g).astype(np.int64)
    kx = np.array([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]], np.int64)
    ix = ndimage.correlate(gi, kx, mode="constant")
    iy = ndimage.correlate(gi, kx.T, mode="constant")
    box = np.ones((7, 7), np.int64)
    a = ndimage.correlate(ix * ix, box, mode="constant").astype(F)
    b = ndimage.correlate(iy * iy, box, mode="constant").astype(F)
    c = ndimage.correlate(ix * iy, box, mode="constant").astype(F)
    sc = F(1) / F(4 * 7 * 255.0)
    s4 = F(F(F(sc * sc) * sc) * sc)
    tr = a + b
    return ((a * b - c * c) - (F(0.04) * tr) * tr) * s4


# ---------------------------------------------------------------------------------------------------- orientation
def umax_from_formula():
    """Upstream's construction of the disc's half-widths: round(sqrt(r^2 - v^2)) up to v = r / sqrt 2, the rest mirrored
    across the diagonal so that the disc is symmetric."""
    r = HALF_PATCH
    umax = np.zeros(r + 2, np.int64)
    vmax = int(np.floor(r * np.sqrt(2.0) / 2 + 1))
    vmin = int(np.ceil(r * np.sqrt(2.0) / 2))
    for v in range(vmax + 1):
        umax[v] = int(np.rint(np.sqrt(float(r * r - v * v))))
    v0 = 0
    for v in range(r, vmin - 1, -1):
        while umax[v0] == umax[v0 + 1]:
            v0 += 1
        umax[v] = v0
        v0 += 1
    return tuple(int(u) for u in umax[:r + 1])


def disc_offsets():
    umax = umax_from_formula()
    assert umax == UMAX_TABLE, umax
    return np.array([(u, v) for v in range(-HALF_PATCH, HALF_PATCH + 1) for u in range(-umax[abs(v)], umax[abs(v)] + 1)], np.int64)


def fast_atan2(y, x):
    """cv::fastAtan2: degrees in [0, 360), a degree-7 odd polynomial of min / max, in float32."""
    y, x = np.asarray(y, F), np.asarray(x, F)
    k = F(180 / np.pi)
    p1, p3, p5, p7 = (F(F(c) * k) for c in (0.9997878412794807, -0.3258083974640975, 0.1555786518463281, -0.04432655554792128))
    ax, ay = np.abs(x), np.abs(y)
    eps = F(2.2204460492503131e-16)
    swap = ax < ay
    c = np.where(swap, ax, ay) / (np.where(swap, ay, ax) + eps)
    c2 = c * c
    a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c
    a = np.where(swap, F(90) - a, a)
    a = np.where(x < 0, F(180) - a, a)
    a = np.where(y < 0, F(360) - a, a)
    return a.astype(F)


def orientation(g, xs, ys):
    """-> (angle degrees float32, dir [n, 2] = (cos, sin) float32): integer moments of the disc, fastAtan2, cos and sin of
    the float32 radians in long double, rounded once."""
    off = disc_offsets()
    patch = np.asarray(g).astype(np.int64)[ys[:, None] + off[None, :, 1], xs[:, None] + off[None, :, 0]]
    m10 = (patch * off[:, 0]).sum(axis=1)
    m01 = (patch * off[:, 1]).sum(axis=1)
    ang = fast_atan2(m01.astype(F), m10.astype(F))
    rad = (ang * F(np.pi / 180.0)).astype(F)
    ld = rad.astype(np.longdouble)
    return ang, np.stack([np.cos(ld).astype(F), np.sin(ld).astype(F)], axis=1)


# ---------------------------------------------------------------------------------------------------- descriptor
def seeded_pattern():
    """The default 256 x 4 pattern (x1 y1 x2 y2): a linear congruential generator, three draws in [-13, 13] summed and
    halved towards zero; a test whose two points coincide has its second x moved one step towards zero."""
    n = 256 * 4 * 3
    s = np.zeros(n, np.uint64)
    cur = 0x9E3779B9
    for i in range(n):
        cur = (cur * 1664525 + 1013904223) & 0xFFFFFFFF
        s[i] = cur
    draws = ((s >> np.uint64(16)) % np.uint64(27)).astype(np.int64) - 13
    acc = draws.reshape(-1, 3).sum(axis=1)
    v = np.clip(np.sign(acc) * (np.abs(acc) // 2), -13, 13).reshape(256, 4)
    same = (v[:, 0] == v[:, 2]) & (v[:, 1] == v[:, 3])
    v[same, 2] = np.where(v[same, 2] >= 0, v[same, 2] - 1, v[same, 2] + 1)
    return v.astype(np.int8)


def describe(blur, xs, ys, dirs, pattern):
    """Steered BRIEF: the pattern rotated by (a, b) in float32 (two products, one sum, each rounded), rounded half to even
    to the pixel grid; test t sets bit t & 31 of word t >> 5 when first < second."""
    a, b = dirs[:, 0:1], dirs[:, 1:2]                                           # [n, 1] float32
    p = np.asarray(pattern, np.int8).reshape(256, 4).astype(F)

    def sample(px, py):
        rx = np.rint(px[None, :] * a - py[None, :] * b).astype(np.int64)
        ry = np.rint(px[None, :] * b + py[None, :] * a).astype(np.int64)
        return np.asarray(blur)[ys[:, None] + ry, xs[:, None] + rx]

    bits = sample(p[:, 0], p[:, 1]) < sample(p[:, 2], p[:, 3])                   # [n, 256]
    weights = (np.uint64(1) << np.arange(32, dtype=np.uint64))
    words = (bits.reshape(len(xs), 8, 32).astype(np.uint64) * weights).sum(axis=2)
    return words.astype(np.uint32)


# ---------------------------------------------------------------------------------------------------- the extractor
def select_level(g, want, fast_t, keep_images=False):
    """Detection and the two retainBest cuts on one level -> (flat pixel indices in raster order, responses, record)."""
    h, w = g.shape
    score = fast_score_image(g, fast_t)
    cand = np.flatnonzero(suppress(score))                                      # raster order
    sc = score.ravel()[cand].astype(np.int64)
    rec = dict(w=w, h=h, want=want, nc=len(cand), fast_cut=0, nk=0, harris_cut=None, ties=0, ties_allowed=0, n=0)
    if keep_images:
        rec["score"], rec["cand"] = score, cand
    # retainBest(2 want) by the FAST score, ties at the cut all kept
    if len(cand) > 2 * want:
        rec["fast_cut"] = int(np.sort(sc)[::-1][2 * want - 1])
        cand = cand[sc >= rec["fast_cut"]]
    rec["nk"] = len(cand)
    resp = harris_image(g).ravel()[cand]
    # retainBest(want) by the response, ties at the cut to the raster-earlier key point
    if len(cand) > want:
        order = np.lexsort((cand, -resp))[:want]
        cut = resp[order[-1]]
        rec["harris_cut"] = float(cut)
        rec["ties"] = int((resp == cut).sum())
        rec["ties_allowed"] = int(want - (resp > cut).sum())
        order = np.sort(order)                                                  # cand is in raster order: so is this
        cand, resp = cand[order], resp[order]
    rec["n"] = len(cand)
    return cand, resp, rec


def orb_extract_cv(img, n_features=500, fast_t=20, n_levels=8, scale_factor=1.2, pattern=None, keep_images=False):
    """-> (xy [n, 2] float32 level-0 pixels, octave [n] int32, response [n] float32, dir [n, 2] float32, angle [n] float32,
    desc [n, 8] uint32), levels (one dict per level that ran: level, w, h, quota, want, nc = candidates after suppression,
    fast_cut, nk = survivors of it, harris_cut, ties at that cut, ties_allowed, n = key points kept)."""
    g = to_gray(img)
    h, w = g.shape
    ws, hs, scales, quota = levels_and_quota(w, h, n_levels, scale_factor, n_features)
    pat = seeded_pattern() if pattern is None else np.asarray(pattern, np.int8).reshape(256, 4)
    out = [[] for _ in range(6)]
    levels, total = [], 0
    for l in range(n_levels):
        if ws[l] <= 2 * EDGE or hs[l] <= 2 * EDGE:
            break                                   # sizes only shrink: no later level has room for a key point either
        if l > 0:
            g = resize_linear(g, int(ws[l]), int(hs[l]))
        want = int(min(quota[l], n_features - total))
        if want <= 0:
            levels.append(dict(level=l, w=int(ws[l]), h=int(hs[l]), quota=int(quota[l]), want=want, nc=None, n=0))
            continue
        idx, resp, rec = select_level(g, want, fast_t, keep_images)
        rec.update(level=l, quota=int(quota[l]))
        levels.append(rec)
        ys, xs = idx // int(ws[l]), idx % int(ws[l])
        ang, dirs = orientation(g, xs, ys)
        desc = describe(gauss7(g), xs, ys, dirs, pat)
        xy = np.stack([xs.astype(F) * scales[l], ys.astype(F) * scales[l]], axis=1).astype(F)
        for o, v in zip(out, (xy, np.full(len(idx), l, np.int32), resp.astype(F), dirs, ang, desc)):
            o.append(v)
        total += len(idx)
    empty = (np.zeros((0, 2), F), np.zeros(0, np.int32), np.zeros(0, F), np.zeros((0, 2), F), np.zeros(0, F), np.zeros((0, 8), np.uint32))
    res = tuple(np.concatenate(o) if o else e for o, e in zip(out, empty))
    return res, levels
