"""The DEFINITION of what csrc/pyramid.hip leaves in device memory, in plain integer numpy: the Gaussian levels, their reflect-101
borders and the packed Scharr derivative levels with their zero border.  Written from the comments of csrc/svo_internal.h (the
layout: SVO_PYR_PAD, SVO_DERIV_PAD, the packing of a derivative word) and from SURVEY.md appendix A.1 (the arithmetic), not from
pyramid.hip and not from oracle/lk.c.  Every comparison against it is exact equality of integers.

`reflect101` here is the LOOP form: any number of folds.  tests/lk_numpy.py::_reflect101 folds once, which is all its callers
need where they are reused here (`pyr_down` reaches two pixels outside a level, `scharr` one, and a level is at least two pixels
wide), so lk_numpy stays as it is; its `_pad_image` with a 23-pixel border is NOT used here, because a single fold is wrong for
a border wider than the level (level 3 of a 44 x 44 image is 6 x 6 under a 32-pixel border)."""
import numpy as np

import lk_numpy


def reflect101(idx, n):
    """cv::borderInterpolate(idx, n, BORDER_REFLECT_101) for any idx: ... 2 1 | 0 1 2 .. n-1 | n-2 n-3 ...; n == 1 gives 0."""
    idx = np.array(idx, np.int64)
    if n == 1:
        return np.zeros_like(idx)
    while True:
        low, high = idx < 0, idx >= n
        if not (low.any() or high.any()):
            return idx
        idx = np.where(low, -idx, idx)
        idx = np.where(idx >= n, 2 * (n - 1) - idx, idx)


def levels(img, n):
    """n levels: the image, then pyrDown of the level before ([1 4 6 4 1]^2 / 256, reflect-101, (sum + 128) >> 8)."""
    out = [np.ascontiguousarray(img)]
    for _ in range(n - 1):
        out.append(lk_numpy.pyr_down(out[-1]))
    return out


def padded(level, pad):
    """The level with a reflect-101 border of `pad` pixels on every side: (h + 2 pad, w + 2 pad, c) uint8."""
    h, w, _ = level.shape
    ys = reflect101(np.arange(-pad, h + pad), h)
    xs = reflect101(np.arange(-pad, w + pad), w)
    return np.ascontiguousarray(level[ys][:, xs])


def derivative_words(level, pad):
    """One int32 per pixel and channel, (4 dx & 0xffff) | (4 dy << 16) of the Scharr derivatives (|4 d| <= 16320 fits int16),
    inside a ZERO border of `pad` pixels: (h + 2 pad, w + 2 pad, c) int32."""
    dx, dy = lk_numpy.scharr(level)
    dx4, dy4 = 4 * dx.astype(np.int64), 4 * dy.astype(np.int64)
    assert np.abs(dx4).max(initial=0) <= 16320 and np.abs(dy4).max(initial=0) <= 16320
    words = ((dx4 & 0xFFFF) | ((dy4 & 0xFFFF) << 16)).astype(np.uint32).view(np.int32)
    return np.pad(words, ((pad, pad), (pad, pad), (0, 0)))


def unpack_words(words):
    """The inverse of the packing: (4 dx, 4 dy) as two int16 planes."""
    u = np.ascontiguousarray(words, np.int32).view(np.uint32)
    return (u & 0xFFFF).astype(np.uint16).view(np.int16), (u >> 16).astype(np.uint16).view(np.int16)


def where_differs(got, want, pad, kind):
    """A sentence for a failure message: the first element that differs, as (row, column, channel) of the UNPADDED level, and
    whether it lies in the interior or in the border; for derivative words also whether dx or dy differs.  None when equal."""
    if got.shape != want.shape:
        return f"shape {got.shape} instead of {want.shape}"
    bad = np.argwhere(got != want)
    if len(bad) == 0:
        return None
    y, x, ch = (int(v) for v in bad[0])
    h, w = want.shape[0] - 2 * pad, want.shape[1] - 2 * pad
    region = "interior" if pad <= y < pad + h and pad <= x < pad + w else "border"
    text = f"{len(bad)} of {want.size} differ, first at row {y - pad}, column {x - pad}, channel {ch} ({region})"
    if kind == "deriv":
        (gx, gy), (wx, wy) = unpack_words(got), unpack_words(want)
        parts = [name for name, g, w_ in (("dx", gx, wx), ("dy", gy, wy)) if (g != w_).any()]
        text += f": {' and '.join(parts)} differ, 4 dx {gx[y, x, ch]} for {wx[y, x, ch]}, 4 dy {gy[y, x, ch]} for {wy[y, x, ch]}"
    else:
        text += f": {got[y, x, ch]} for {want[y, x, ch]}"
    return text
