"""A blind numpy restatement of cv::FAST (TYPE_9_16) as DESIGN.md section 10j defines it, the second party beside the HIP kernels
(csrc/fast.hip).

TEST INFRASTRUCTURE.  Written from the definition -- the FAST paper's segment test (Rosten & Drummond 2006), "the score is the
largest threshold at which the pixel still fires", suppression against the eight neighbours, KeyPointsFilter::retainBest -- and NOT
from the kernel: whole images at a time, the arcs by their definition (an index table of 16 starts x 9 members), selection through
np.nonzero and np.sort.  It shares nothing with tests/orb_numpy.py except the order of the ring, which it restates;
tests/test_fast_numpy.py holds the two score planes against each other.

fast_detect(img, threshold, nonmax, max_keypoints) -> (xy [n, 2] float32, response [n] float32, score [h, w] uint8)
"""
import numpy as np

# the 16 pixels of the radius-3 Bresenham circle, clockwise from twelve o'clock: (dx, dy)
RING = ((0, -3), (1, -3), (2, -2), (3, -1), (3, 0), (3, 1), (2, 2), (1, 3),
        (0, 3), (-1, 3), (-2, 2), (-3, 1), (-3, 0), (-3, -1), (-2, -2), (-1, -3))
ARCS = (np.arange(16)[:, None] + np.arange(9)[None, :]) % 16          # [start, member]
BORDER = 3


def to_gray(img):
    """cvtColor(BGR2GRAY)'s integer weights (14 fractional bits, one rounding); one channel passes through."""
    img = np.asarray(img, np.uint8)
    if img.ndim == 2:
        return img.copy()
    if img.shape[2] == 1:
        return img[..., 0].copy()
    b, g, r = (img[..., k].astype(np.int64) for k in range(3))
    return ((1868 * b + 9617 * g + 4899 * r + 8192) >> 14).astype(np.uint8)


def _ring_minus_centre(g):
    """int32 [h - 6, w - 6, 16] for the pixels whose ring lies inside the image; None when there are none."""
    g = np.asarray(g).astype(np.int32)
    h, w = g.shape
    if h < 2 * BORDER + 1 or w < 2 * BORDER + 1:
        return None
    c = g[BORDER:h - BORDER, BORDER:w - BORDER]
    return np.stack([g[BORDER + dy:h - BORDER + dy, BORDER + dx:w - BORDER + dx] - c for dx, dy in RING], axis=-1)


def fires(g, t):
    """The segment test at threshold t -> bool [h, w]: nine cyclically contiguous ring pixels all > centre + t, or all
    < centre - t; False where the ring leaves the image."""
    t = min(max(int(t), 0), 255)
    out = np.zeros(np.asarray(g).shape, bool)
    d = _ring_minus_centre(g)
    if d is None:
        return out
    brighter, darker = d > t, d < -t
    out[BORDER:-BORDER, BORDER:-BORDER] = brighter[..., ARCS].all(-1).any(-1) | darker[..., ARCS].all(-1).any(-1)
    return out


def arc_best(g):
    """int32 [h, w]: over the 16 arcs of nine, the largest of min(ring - centre) and of min(centre - ring); -256 where the ring
    leaves the image.  A pixel fires at t exactly when this exceeds t."""
    out = np.full(np.asarray(g).shape, -256, np.int32)
    d = _ring_minus_centre(g)
    if d is None:
        return out
    arcs = d[..., ARCS]                                                  # [h - 6, w - 6, 16, 9]
    out[BORDER:-BORDER, BORDER:-BORDER] = np.maximum(arcs.min(-1).max(-1), (-arcs).min(-1).max(-1))
    return out


def score_image(g, t):
    """uint8 [h, w]: the corner score (arc_best - 1) where the pixel fires at t, 0 elsewhere and on the border."""
    return np.where(fires(g, t), arc_best(g) - 1, 0).astype(np.uint8)


def suppress(fired, score):
    """bool [h, w]: corners whose score is strictly above the scores of all eight neighbours; a neighbour that is no corner (the
    border included) counts 0."""
    s = np.where(fired, score.astype(np.int32), 0)
    p = np.pad(s, 1)                                                     # the image's own edge never fires: the pad value is unused
    keep = fired.copy()
    h, w = s.shape
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                keep &= s > p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    return keep


def retain_best(xy, response, n_points):
    """KeyPointsFilter::retainBest: with more than n_points key points, keep every one whose response is at or above the
    n_points-th largest (ties included), in the order they came."""
    if n_points <= 0 or len(response) <= n_points:
        return xy, response
    cut = np.sort(response)[::-1][n_points - 1]
    keep = response >= cut
    return xy[keep], response[keep]


def fast_detect(img, threshold=10, nonmax=True, max_keypoints=0):
    g = to_gray(img)
    t = min(max(int(threshold), 0), 255)
    f = fires(g, t)
    score = score_image(g, t)
    keep = suppress(f, score) if nonmax else f
    ys, xs = np.nonzero(keep)                                            # row-major: y ascending, then x
    xy = np.stack([xs, ys], axis=-1).astype(np.float32).reshape(-1, 2)
    response = score[ys, xs].astype(np.float32) if nonmax else np.zeros(len(xs), np.float32)
    xy, response = retain_best(xy, response, max_keypoints)
    return xy, response, score
