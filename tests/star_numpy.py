"""The Star (CenSurE) detector, stated operation by operation in numpy -- the definition csrc/star.hip is held to bit for bit
(DESIGN.md section 10m).  OpenCV 3.2's xfeatures2d::StarDetector::detect as recalled; nothing here was run against upstream.

S1  grey: the image itself (c = 1) or cvtColor's integer weights on B, G, R (c = 3).
S2  tables: SIZES0, PAIRS (outer index, inner index); for an index i, r = SIZES0[i] and t = r + r // 2.
S3  pattern count (layout): n counts up while n < 12, SIZES0[PAIRS[n][0]] < max_size and (n + 1 == 12 or
    t(PAIRS[n + 1][0]) < min(w, h)); npatterns = min(n + 1, 12) -- OURS-1: upstream reads past its tables when max_size > 90 --,
    max_idx = PAIRS[npatterns - 1][0], border = t(max_idx).
S4  star sum vals[i](x, y): grey over the square |dx|, |dy| <= r plus grey over the diamond |dx| + |dy| <= t, the overlap counted
    twice; area[i] = (2 r + 1)^2 + t^2 + (t + 1)^2.  int32, exact.  Here: an upright integral image and two diagonal-cone tables.
S5  response / size planes (float32 / int16), zero outside border <= x < w - border, border <= y < h - border; inside, over the
    patterns in order, resp = float(inner) * (1.f / innerArea) - float(outer) * (1.f / outerArea) in float32, one multiply, one
    multiply, one subtract; the strictly largest |resp| wins (start: 0, size 0), the earliest on ties.
S6  suppression: tiles of (delta + 1)^2 pixels, delta = suppress_nonmax_size // 2, anchored at (border, border); per tile the
    strict maximum above float(response_threshold) and, among the pixels that are no new maximum, the strict minimum below
    -float(response_threshold); a candidate falls when another pixel of its (2 delta + 1)^2 neighbourhood (clipped to the image)
    is >= (<=) it; it must have size >= 4 and pass the line test.  A tile emits its maximum before its minimum, tiles in
    row-major order.
S7  line test: d = sz // 4, samples u, v in {-4 d, ..., 4 d} step d (v outer), central differences of the response plane summed in
    float32 in sample order; fires when (Lxx + Lyy)^2 >= float(line_threshold_projected) * (Lxx Lyy - Lxy^2); else the same in
    int32 on (size == sz) with line_threshold_binarized.
"""
import numpy as np

F = np.float32

SIZES0 = (1, 2, 3, 4, 6, 8, 11, 12, 16, 22, 23, 32, 45, 46, 64, 90, 128)
PAIRS = ((1, 0), (3, 1), (4, 2), (5, 3), (7, 4), (8, 5), (9, 6), (11, 8), (13, 10), (14, 11), (15, 12), (16, 14))
DEFAULTS = dict(max_size=45, response_threshold=30, line_threshold_projected=10, line_threshold_binarized=8, suppress_nonmax_size=5)


def tilt(i):
    return SIZES0[i] + SIZES0[i] // 2


def area(i):
    r, t = SIZES0[i], tilt(i)
    return (2 * r + 1) ** 2 + t * t + (t + 1) ** 2


def layout(w, h, max_size):
    """S3 -> (npatterns, max_idx, border)."""
    n = 0
    while n < 12 and SIZES0[PAIRS[n][0]] < max_size and (n + 1 == 12 or tilt(PAIRS[n + 1][0]) < min(w, h)):
        n += 1
    npatterns = min(n + 1, 12)
    max_idx = PAIRS[npatterns - 1][0]
    return npatterns, max_idx, tilt(max_idx)


def grey(img):
    img = np.asarray(img, np.uint8)
    if img.ndim == 2:
        return img.astype(np.int64)
    b, g, r = (img[..., k].astype(np.int64) for k in range(3))
    return (b * 1868 + g * 9617 + r * 4899 + 8192) >> 14


def tables(g):
    """The upright integral image [h + 1, w + 1] and the two cone tables [h + 1, w + 1], entry [y + 1, x + 1] for the apex (x, y),
    x = -1 ... w - 1: even(x, y) = sum over y' <= y, |x' - x| <= y - y'; odd(x, y) = sum over y' <= y, x - k <= x' <= x + 1 + k,
    k = y - y'."""
    h, w = g.shape
    up = np.zeros((h + 1, w + 1), np.int64)
    up[1:, 1:] = g.cumsum(0).cumsum(1)
    gp = np.zeros((h, w + 2), np.int64)           # column j = pixel x = j - 1
    gp[:, 1:w + 1] = g
    dl = np.zeros((h, w + 2), np.int64)           # the diagonal that ends at (x, y) coming from the upper left
    dr = np.zeros((h, w + 2), np.int64)           # ... from the upper right
    for y in range(h):
        dl[y] = gp[y]
        dr[y] = gp[y]
        if y:
            dl[y, 1:] += dl[y - 1, :-1]
            dr[y, :-1] += dr[y - 1, 1:]
    even = np.zeros((h + 1, w + 1), np.int64)
    odd = np.zeros((h + 1, w + 1), np.int64)
    even[1:] = (dl + dr - gp)[:, :w + 1].cumsum(0)
    odd[1:] = (dl[:, :w + 1] + dr[:, 1:]).cumsum(0)
    return up, even, odd


def star_sums(g, i, border):
    """S4 for every pixel with border <= x < w - border, border <= y < h - border -> [h - 2 border, w - 2 border] int64."""
    h, w = g.shape
    up, even, odd = tables(g)
    r, t = SIZES0[i], tilt(i)
    ys, xs = np.mgrid[border:h - border, border:w - border]
    sq = up[ys + r + 1, xs + r + 1] - up[ys - r, xs + r + 1] - up[ys + r + 1, xs - r] + up[ys - r, xs - r]
    E = lambda x, y: even[y + 1, x + 1]
    O = lambda x, y: odd[y + 1, x + 1]
    di = E(xs, ys + t) - O(xs - t - 1, ys - 1) - O(xs + t, ys - 1) + E(xs, ys - t - 1)
    return sq + di


def responses(img, max_size=45):
    """S5 -> (response [h, w] float32, size [h, w] int16, border, winning pattern [h, w] int8, -1 where none)."""
    g = grey(img)
    h, w = g.shape
    assert 255 * w * h <= 2 ** 31 - 1
    npat, max_idx, border = layout(w, h, max_size)
    resp, size = np.zeros((h, w), F), np.zeros((h, w), np.int16)
    win = np.full((h, w), -1, np.int8)
    if w <= 2 * border or h <= 2 * border:
        return resp, size, border, win
    need = sorted({i for p in PAIRS[:npat] for i in p})
    vals = {i: star_sums(g, i, border) for i in need}
    best, bsz = np.zeros((h - 2 * border, w - 2 * border), F), np.zeros((h - 2 * border, w - 2 * border), np.int16)
    bwin = np.full(best.shape, -1, np.int8)
    for p in range(npat):
        o, i = PAIRS[p]
        inner = vals[i]
        outer = vals[o] - inner
        inv_i, inv_o = F(1) / F(area(i)), F(1) / F(area(o) - area(i))
        r = inner.astype(F) * inv_i - outer.astype(F) * inv_o
        assert r.dtype == F
        m = np.abs(r) > np.abs(best)
        best, bsz, bwin = np.where(m, r, best), np.where(m, np.int16(SIZES0[o]), bsz), np.where(m, np.int8(p), bwin)
    resp[border:h - border, border:w - border] = best
    size[border:h - border, border:w - border] = bsz
    win[border:h - border, border:w - border] = bwin
    return resp, size, border, win


def line_test(resp, size, x, y, sz, lt_proj, lt_bin, record=None):
    """S7 -> True when the candidate lies on a line."""
    h, w = resp.shape
    R = lambda xx, yy: resp[yy, xx] if 0 <= xx < w and 0 <= yy < h else F(0)
    B = lambda xx, yy: int(size[yy, xx] == sz) if 0 <= xx < w and 0 <= yy < h else 0
    d = sz // 4
    offs = range(-4 * d, 4 * d + 1, d)
    lxx = lyy = lxy = F(0)
    for v in offs:
        for u in offs:
            lx = F(R(x + u + 1, y + v) - R(x + u - 1, y + v))
            ly = F(R(x + u, y + v + 1) - R(x + u, y + v - 1))
            lxx = F(lxx + F(lx * lx))
            lyy = F(lyy + F(ly * ly))
            lxy = F(lxy + F(lx * ly))
    s = F(lxx + lyy)
    if F(s * s) >= F(F(lt_proj) * F(F(lxx * lyy) - F(lxy * lxy))):
        if record is not None:
            record["line_projected"] += 1
        return True
    bxx = byy = bxy = 0
    for v in offs:
        for u in offs:
            lx = B(x + u + 1, y + v) - B(x + u - 1, y + v)
            ly = B(x + u, y + v + 1) - B(x + u, y + v - 1)
            bxx += lx * lx
            byy += ly * ly
            bxy += lx * ly
    if (bxx + byy) * (bxx + byy) >= lt_bin * (bxx * byy - bxy * bxy):
        if record is not None:
            record["line_binarized"] += 1
        return True
    return False


def detect(img, max_size=45, response_threshold=30, line_threshold_projected=10, line_threshold_binarized=8,
           suppress_nonmax_size=5, record=None):
    """S1 ... S7 -> (xy [n, 2] float32, size [n] float32, response [n] float32) in the stated order.  `record`, a dict, counts what
    happened: maxima, minima, and the candidates each rule removed."""
    resp, size, border, win = responses(img, max_size)
    h, w = resp.shape
    if record is not None:
        for k in ("max_kept", "min_kept", "neighbourhood", "neighbourhood_equal", "size_rule","line_projected", "line_binarized", "candidates"):
            record.setdefault(k, 0)
        record.setdefault("patterns_won", set()).update(int(p) for p in np.unique(win) if p >= 0)
    delta = suppress_nonmax_size // 2
    out = []
    for y0 in range(border, h - border, delta + 1):
        for x0 in range(border, w - border, delta + 1):
            hi, lo = F(response_threshold), F(-F(response_threshold))
            pmax = pmin = None
            for y in range(y0, min(y0 + delta + 1, h - border)):
                for x in range(x0, min(x0 + delta + 1, w - border)):
                    v = resp[y, x]
                    if v > hi:
                        hi, pmax = v, (x, y)
                    elif v < lo:
                        lo, pmin = v, (x, y)
            for pt, ext, is_max in ((pmax, hi, True), (pmin, lo, False)):
                if pt is None:
                    continue
                x, y = pt
                if record is not None:
                    record["candidates"] += 1
                ya, yb, xa, xb = max(y - delta, 0), min(y + delta, h - 1), max(x - delta, 0), min(x + delta, w - 1)
                nb = resp[ya:yb + 1, xa:xb + 1]
                hits = int((nb >= ext).sum()) if is_max else int((nb <= ext).sum())
                if hits > 1:                       # the candidate itself is one
                    if record is not None:
                        record["neighbourhood"] += 1
                        beyond = int((nb > ext).sum()) if is_max else int((nb < ext).sum())
                        record["neighbourhood_equal"] += beyond == 0      # removed by an equal response alone
                    continue
                sz = int(size[y, x])
                if sz < 4:
                    if record is not None:
                        record["size_rule"] += 1
                    continue
                if line_test(resp, size, x, y, sz, line_threshold_projected, line_threshold_binarized, record):
                    continue
                if record is not None:
                    record["max_kept" if is_max else "min_kept"] += 1
                out.append((x, y, sz, ext))
    xy = np.array([(o[0], o[1]) for o in out], F).reshape(-1, 2)
    return xy, np.array([o[2] for o in out], F), np.array([o[3] for o in out], F)
