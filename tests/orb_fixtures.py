"""Seeded images that steer the extractor in cv::ORB's shape into the branches the corridor scene never reaches
(tests/test_orb_numpy.py on the CPU, tests/test_gpu_orb_edges.py on the GPU).  Every image is at most 400 x 320; what each
one must reach is asserted by those tests from orb_numpy's per-level record, so a generator that drifts fails loudly."""
import functools

import numpy as np
from scipy import ndimage

W, H = 384, 320                     # the size the motif, ramp and noise images share (one extractor serves all three)
TILE_W, TILE_H = 128, 16            # the detector's tile: borders at multiples of these


def motif(w=W, h=H, seed=11):
    """A 7 x 7 motif tiled over the image (7 divides neither 128 nor 16): one pixel of 150 on a background of 0..9 and one of
    40.  Every period holds one corner of the same FAST score and the same Harris response."""
    rng = np.random.default_rng(seed)
    m = rng.integers(0, 10, (7, 7)).astype(np.uint8)
    m[0, 0] = 150
    m[1, 2] = 40
    return np.tile(m, (h // 7 + 1, w // 7 + 1))[:h, :w].copy()


def motif_ramp(w=W, h=H, seed=11):
    """The motif with a gentle ramp added over the right half, half a grey level per pixel and a whole one in the top 60
    rows: the responses there leave the common value, some above it, so that the Harris cut falls inside a run of equals."""
    g = motif(w, h, seed).astype(np.int64)
    x = np.maximum(np.arange(w) - w // 2, 0)
    ramp = np.where(np.arange(h)[:, None] < 60, np.minimum(x, 100)[None, :], (x // 2)[None, :])
    return np.minimum(g + ramp, 255).astype(np.uint8)


def sparse(w=400, h=320, seed=5, n_blobs=30):
    """About 30 isolated Gaussian blobs of random height and width on a flat background."""
    rng = np.random.default_rng(seed)
    img = np.full((h, w), 40.0)
    yy, xx = np.mgrid[0:h, 0:w]
    for _ in range(n_blobs):
        cx, cy = rng.uniform(40, w - 40), rng.uniform(40, h - 40)
        s, a = rng.uniform(1.2, 3.0), rng.uniform(80, 200)
        img += a * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * s * s))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def noise3(w=W, h=H, seed=0):
    """Pixels drawn from {0, 128, 255} at half size, doubled: 2 x 2 plateaus, corners nearly everywhere at threshold 1."""
    rng = np.random.default_rng(seed)
    half = np.array([0, 128, 255], np.uint8)[rng.integers(0, 3, ((h + 1) // 2, (w + 1) // 2))]
    return np.kron(half, np.ones((2, 2), np.uint8))[:h, :w].copy()


def flat(w=W, h=H, value=77):
    return np.full((h, w), value, np.uint8)


GEOMETRY_SIZES = ((63, 63), (70, 140), (129, 80), (131, 97), (257, 66), (200, 63))      # w x h; 63 = the smallest accepted


def geometry(w, h, seed=3):
    """Smoothed noise stretched to the full range, with a lone bright pixel at (31, 31): the one place where a 63-pixel
    side can hold a key point at all."""
    rng = np.random.default_rng(seed + 1000 * w + h)
    g = ndimage.gaussian_filter(rng.uniform(0, 1, (h, w)), 1.0)
    g = (g - g.min()) / (g.max() - g.min()) * 255
    g[28:35, 28:35] = 10
    g[31, 31] = 250
    return np.rint(g).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def crop_400x220():
    """The 400 x 220 grey crop of the corridor scene that tests/test_gpu_orb.py uses."""
    import orb_numpy
    from ros_stereo_slam_amd import synth

    R, t = synth.corridor_trajectory(3)[2]
    return orb_numpy.to_gray(synth.Scene().stereo(R, t)[0])[40:260, 100:500].copy()


def random_pattern(seed=41):
    """A 256 x 4 sampling pattern with entries up to +-15 (the corners of the 31-pixel patch included), no test on one pixel."""
    rng = np.random.default_rng(seed)
    pat = rng.integers(-15, 16, (256, 4)).astype(np.int8)
    pat[0], pat[1] = (15, 15, -15, -15), (-15, 15, 15, -15)
    same = (pat[:, 0] == pat[:, 2]) & (pat[:, 1] == pat[:, 3])
    pat[same, 2] = np.where(pat[same, 2] >= 0, pat[same, 2] - 1, pat[same, 2] + 1)
    return pat


def _p(n_features, fast_t, n_levels, scale_factor):
    return dict(n_features=n_features, fast_t=fast_t, n_levels=n_levels, scale_factor=scale_factor)


def cases():
    """name -> (image maker, parameters of the extractor)."""
    c = {
        "motif": (motif, _p(200, 20, 1, 1.2)),
        "motif_ramp": (motif_ramp, _p(200, 20, 1, 1.2)),
        "sparse": (sparse, _p(500, 20, 8, 1.2)),
        "noise3": (noise3, _p(1000, 1, 3, 1.2)),
    }
    for w, h in GEOMETRY_SIZES:
        for sf in (1.2, 2.0):
            c[f"geom_{w}x{h}_x{sf}"] = (functools.partial(geometry, w, h), _p(300, 20, 8, sf))
    c["geom_257x66_x2.5"] = (functools.partial(geometry, 257, 66), _p(300, 20, 8, 2.5))
    c["geom_200x63_x2.5"] = (functools.partial(geometry, 200, 63), _p(300, 20, 8, 2.5))
    for nf in (1, 7, 8):
        c[f"budget_{nf}"] = (crop_400x220, _p(nf, 20, 8, 1.2))
    return c


@functools.lru_cache(maxsize=None)
def reference(name, random=False):
    """orb_numpy on one case, computed once and shared: -> (image, parameters, pattern or None, the six outputs, levels).
    Nobody writes into what this returns."""
    import orb_numpy

    make, prm = cases()[name]
    img = make()
    pat = random_pattern() if random else None
    res, levels = orb_numpy.orb_extract_cv(img, pattern=pat, keep_images=True, **prm)
    return img, prm, pat, res, levels
