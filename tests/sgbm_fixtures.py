"""Input generators of tests/test_gpu_sgbm_edges.py: pairs that drive the matcher into the corners a smooth texture
never reaches (saturated sums, wrapped int16 costs, ties everywhere)."""
import numpy as np

from ros_stereo_slam_amd import synth


def unrelated(w, h, seed=0, run=1):
    """Independent random 0/255 images, constant over horizontal runs of ``run`` pixels: every pixel cost is large and
    block sums saturate S.  Birchfield-Tomasi's half-sample interval forgives single-pixel noise; runs of 3 are what
    keeps a share of the pixels saturated at every d once D is large."""
    rng = np.random.default_rng(seed)

    def one():
        return (rng.integers(0, 2, (h, -(-w // run))).repeat(run, 1)[:, :w] * 255).astype(np.uint8)

    return one(), one()


def textured(w, h, shift=5, seed=1, noise=6, c=1):
    """The noisy shifted texture of test_gpu_sgbm.py's ``_pair``: h x w for c = 1, else h x w x c."""
    a, b = synth.textured_pair(w, h, c, shift=(shift, 0), seed=seed, colour=c == 3)
    rng = np.random.default_rng(seed)
    left = np.clip(b.astype(np.int32) + rng.integers(-noise, noise + 1, b.shape), 0, 255).astype(np.uint8)
    right = np.clip(a.astype(np.int32) + rng.integers(-noise, noise + 1, a.shape), 0, 255).astype(np.uint8)
    return (left[..., 0], right[..., 0]) if c == 1 else (left, right)


def mixed(w, h, seed=0):
    """The left half a matched texture, the right half unrelated 0/255 noise: low and saturating costs in one row."""
    left, right = textured(w, h, seed=seed + 1)
    left, right = left.copy(), right.copy()
    ul, ur = unrelated(w, h, seed)
    left[:, w // 2:], right[:, w // 2:] = ul[:, w // 2:], ur[:, w // 2:]
    return left, right


def constant(w, h, value=61):
    """Every cost of every disparity ties.  61 is ftzero of the default cap, the value R2 writes into columns 0 and
    w - 1 of both channels: the filtered images are constant up to the border, so S is 0 at every d of every pixel."""
    img = np.full((h, w), value, np.uint8)
    return img, img.copy()


def stripes(w, h, period=8, roll=3, offset=8):
    """Vertical stripes with a period shorter than D, the right image rolled by ``roll``: d and d + period tie.  The
    right image is ``offset`` brighter, so the tied minimum is above 0 and the uniqueness product has something to drop."""
    row = np.where((np.arange(w) % period) < period // 2, 40, 210).astype(np.uint8)
    left = np.repeat(row[None], h, 0)
    return left, np.ascontiguousarray(np.roll(left, -roll, 1) + np.uint8(offset))


def half_stripes(w, h):
    """A matched texture on the left three fifths, ``stripes`` on the rest: unique minima and tied ones in one row, so
    a uniqueness ratio drops some pixels and keeps others."""
    left, right = stripes(w, h)
    tl, tr = textured(w, h, shift=3, seed=5)
    k = 3 * w // 5
    left[:, :k], right[:, :k] = tl[:, :k], tr[:, :k]
    return left, right
