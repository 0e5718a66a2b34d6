"""OpenCV 3.2's xfeatures2d::BriefDescriptorExtractor::compute restated in numpy: the yardstick
ros_stereo_slam_amd/csrc/brief.hip is held to bit for bit (tests/test_gpu_brief.py).  The points B1 ... B7 are recalled from
xfeatures2d/src/brief.cpp; OURS-1 is this project's own.

B1  PATCH_SIZE 48, KERNEL_SIZE 9, HALF_KERNEL 4; 16, 32 or 64 bytes, 8 tests per byte; no use_orientation.
B2  a 3-channel image goes through cvtColor(BGR2GRAY): (1868 B + 9617 G + 4899 R + 8192) >> 14.
B3  integral(grey, sum, CV_32S): (h + 1) x (w + 1) int32, zero first row and column.
B4  KeyPointsFilter::runByImageBorder(kps, size, 28): nothing stays when w <= 56 or h <= 56; otherwise a key point stays when
    Rect(28, 28, w - 56, h - 56) contains Point(cvRound(x), cvRound(y)) -- round half to even; the order is preserved.
OURS-1  a kept key point with (int)(x + 0.5) > w - 29 or (int)(y + 0.5) > h - 29 is removed too (a half-integer coordinate on
    the far border: upstream reads one column or row past the integral image there with an offset of +24).
B5  smoothed sample at offset (y, x): iy = (int)(pt.y + 0.5) + y, ix = (int)(pt.x + 0.5) + x -- the sum in double, truncated --,
    S = sum[iy + 5][ix + 5] - sum[iy + 5][ix - 4] - sum[iy - 4][ix + 5] + sum[iy - 4][ix - 4].
B6  test t = (y1, x1, y2, x2): bit S(y1, x1) < S(y2, x2) at bit 7 - t % 8 of byte t / 8; one row per kept key point.
B7  the test table is a parameter: 8 * bytes rows of four int8, every entry in -24 ... 24, (y1, x1) != (y2, x2)."""
import numpy as np

PATCH_SIZE, KERNEL_SIZE, HALF_KERNEL, BORDER = 48, 9, 4, 28


def to_grey(img):
    """B2"""
    img = np.asarray(img, np.uint8)
    if img.ndim == 2:
        return img
    if img.shape[2] == 1:
        return img[..., 0]
    b, g, r = (img[..., k].astype(np.int64) for k in range(3))
    return ((1868 * b + 9617 * g + 4899 * r + 8192) >> 14).astype(np.uint8)


def integral(grey):
    """B3"""
    h, w = grey.shape
    s = np.zeros((h + 1, w + 1), np.int64)
    s[1:, 1:] = np.cumsum(np.cumsum(grey.astype(np.int64), axis=0), axis=1)
    assert s.max() < 2 ** 31
    return s.astype(np.int32)


def centres(xy):
    """B5: (int)(pt + 0.5), the sum in double; only meaningful for key points the filter keeps"""
    with np.errstate(invalid="ignore"):
        return np.trunc(np.asarray(xy, np.float32).reshape(-1, 2).astype(np.float64) + 0.5)


def keep_mask(xy, w, h):
    """B4 and OURS-1 -> bool per key point"""
    p = np.asarray(xy, np.float32).reshape(-1, 2).astype(np.float64)
    if w <= 2 * BORDER or h <= 2 * BORDER:
        return np.zeros(len(p), bool)
    with np.errstate(invalid="ignore"):
        r = np.rint(p)   # cvRound: half to even
        keep = (r[:, 0] >= BORDER) & (r[:, 0] < w - BORDER) & (r[:, 1] >= BORDER) & (r[:, 1] < h - BORDER)
        c = centres(xy)
        keep &= (c[:, 0] <= w - BORDER - 1) & (c[:, 1] <= h - BORDER - 1)   # OURS-1
    return keep


def check_table(table, nbytes):
    """B7"""
    t = np.asarray(table)
    assert nbytes in (16, 32, 64) and t.shape == (8 * nbytes, 4)
    assert np.abs(t.astype(np.int64)).max() <= PATCH_SIZE // 2
    assert not np.any((t[:, 0] == t[:, 2]) & (t[:, 1] == t[:, 3]))
    return t.astype(np.int64)


def smoothed(s, iy, ix):
    """B5: the box sums at integer centres (arrays of equal shape)"""
    s = s.astype(np.int64)
    a, b = HALF_KERNEL + 1, HALF_KERNEL
    return s[iy + a, ix + a] - s[iy + a, ix - b] - s[iy - b, ix + a] + s[iy - b, ix - b]


def describe(img, xy, table, nbytes=32, chunk=4096):
    """compute(img, keypoints) -> (desc [m, nbytes] uint8, kept_index [m] int32)"""
    t = check_table(table, nbytes)
    grey = to_grey(img)
    h, w = grey.shape
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    kept = np.flatnonzero(keep_mask(xy, w, h)).astype(np.int32)
    desc = np.zeros((len(kept), nbytes), np.uint8)
    if len(kept) == 0:
        return desc, kept
    s = integral(grey)
    c = centres(xy[kept]).astype(np.int64)
    for a in range(0, len(kept), chunk):
        cx, cy = c[a:a + chunk, 0][:, None], c[a:a + chunk, 1][:, None]
        s1 = smoothed(s, cy + t[None, :, 0], cx + t[None, :, 1])
        s2 = smoothed(s, cy + t[None, :, 2], cx + t[None, :, 3])
        desc[a:a + chunk] = np.packbits(s1 < s2, axis=1, bitorder="big")   # B6: test 8 b + k at bit 7 - k of byte b
    return desc, kept
