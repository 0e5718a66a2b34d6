"""The batched detector wrappers of ros_stereo_slam_amd/capi.py through the call they share (_batch_call): host images against device
images bit for bit -- the device path carves its columns out of one buffer, so a pointer / view mismatch shows here --, batches of 1
and 3 with an image without texture in the middle, the runs without descriptors, the capacity errors and FAST's score plane.  What
the kernels compute is the business of test_gpu_{sift,surf,fast,star,brief}.py; every comparison here is exact."""
import functools

import numpy as np
import pytest

from ros_stereo_slam_amd import capi, synth

pytestmark = pytest.mark.gpu

W, H = 160, 120
STAR = dict(max_size=16, response_threshold=10)      # the default max_size leaves no interior in an image this small
CAP = 2000                                           # above every count of these images (asserted below)


@functools.lru_cache(maxsize=None)
def textured(seed):
    return np.ascontiguousarray(synth.textured_pair(W, H, 1, seed=seed, wavelength=3.0)[0].reshape(H, W))


@functools.lru_cache(maxsize=None)
def batch(nimg):
    """1, 2 or 3 host images; the middle one of 3 is flat, so its count is 0 between two that are not"""
    flat = np.full((H, W), 128, np.uint8)
    return {1: (textured(1),), 2: (textured(1), textured(2)), 3: (textured(1), flat, textured(2))}[nimg]


def on_device(images):
    import torch

    return [torch.from_numpy(im).cuda() for im in images]


@functools.lru_cache(maxsize=None)
def brief_points(nimg):
    """up to 100 of the restated FAST's corners per image, spread over the rows, so that some lie inside BRIEF's border and some do
    not; none for the flat image"""
    import fast_numpy

    corners = [fast_numpy.fast_detect(im, 10, True, 0)[0] for im in batch(nimg)]
    return tuple(np.ascontiguousarray(xy[::max(len(xy) // 100, 1)][:100], np.float32) for xy in corners)


DETECTORS = {
    "sift_extract": lambda ctx, ims, **kw: ctx.sift_extract(ims, **{"cap": CAP, **kw}),
    "surf_extract": lambda ctx, ims, **kw: ctx.surf_extract(ims, **{"cap": CAP, **kw}),
    "fast_detect": lambda ctx, ims, **kw: ctx.fast_detect(ims, **kw),
    "fast_anms": lambda ctx, ims, **kw: ctx.fast_anms(ims, 50, **kw),
    "star_detect": lambda ctx, ims, **kw: ctx.star_detect(ims, STAR, **kw),
    "brief_describe": lambda ctx, ims, **kw: ctx.brief_describe(ims, list(brief_points(len(ims))), **kw),
}
# the arrays per image, and their dtypes
COLUMNS = {
    "sift_extract": [np.float32] * 4 + [np.int32, np.float32],
    "surf_extract": [np.float32] * 4 + [np.int32, np.int32, np.float32],
    "fast_detect": [np.float32] * 2,
    "fast_anms": [np.float32] * 2,
    "star_detect": [np.float32] * 3,
    "brief_describe": [np.uint8, np.int32],
}


def assert_same(got, want, what):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w), (what, i)
        for j, (a, b) in enumerate(zip(g, w)):
            if a is None or b is None:
                assert a is None and b is None, (what, i, j)
                continue
            assert a.dtype == b.dtype and a.shape == b.shape, (what, i, j, a.dtype, b.dtype, a.shape, b.shape)
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (what, i, j)


@functools.lru_cache(maxsize=None)
def host_run(ctx, name, nimg):
    return DETECTORS[name](ctx, list(batch(nimg)))


@pytest.mark.parametrize("nimg", [2, 1, 3])
@pytest.mark.parametrize("name", sorted(DETECTORS))
def test_host_images_equal_device_images(ctx, name, nimg):
    host = host_run(ctx, name, nimg)
    dev = DETECTORS[name](ctx, on_device(batch(nimg)))
    assert len(host) == nimg
    for per_image in host:
        assert [a.dtype for a in per_image] == COLUMNS[name]
        assert len({len(a) for a in per_image}) == 1
    assert_same(dev, host, name)
    counts = [len(r[0]) for r in host]
    assert all(0 < k < CAP for k in counts[::2]), counts
    if nimg == 3:
        assert counts[1] == 0, counts
        # an image's result does not depend on its place in the batch
        assert_same(host[:1], host_run(ctx, name, 1), name)
        assert_same([host[0], host[2]], host_run(ctx, name, 2), name)


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("name", ["sift_extract", "surf_extract"])
def test_without_descriptors(ctx, name, device):
    images = on_device(batch(3)) if device else list(batch(3))
    bare = DETECTORS[name](ctx, images, descriptors=False)
    full = host_run(ctx, name, 3)
    assert all(r[-1] is None for r in bare) and all(r[-1] is not None and r[-1].shape[1] in (64, 128) for r in full)
    assert_same([r[:-1] for r in bare], [r[:-1] for r in full], name)


def small_cap(counts):
    cap = max(counts) // 2
    assert 0 < cap < max(counts), counts            # the fullest image exceeds it
    return cap


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("name", ["sift_extract", "fast_detect", "star_detect"])
def test_capacity_error_carries_the_counts(ctx, name, device):
    counts = [len(r[0]) for r in host_run(ctx, name, 3)]
    images = on_device(batch(3)) if device else list(batch(3))
    with pytest.raises(capi.SvoError) as ei:
        DETECTORS[name](ctx, images, cap=small_cap(counts))
    assert ei.value.code == capi.SVO_ERR_CAPACITY and ei.value.needed == counts
    assert not hasattr(ei.value, "prefix") and str(ei.value).startswith(f"libsvo_hip error {capi.SVO_ERR_CAPACITY}: ")
    # the context is as good as before
    assert_same(DETECTORS[name](ctx, images), host_run(ctx, name, 3), name)


@pytest.mark.parametrize("descriptors", [True, False])
@pytest.mark.parametrize("device", [False, True])
def test_surf_capacity_error_carries_the_prefix(ctx, device, descriptors):
    full = host_run(ctx, "surf_extract", 3)
    counts = [len(r[0]) for r in full]
    cap = small_cap(counts)
    images = on_device(batch(3)) if device else list(batch(3))
    with pytest.raises(capi.SvoError) as ei:
        ctx.surf_extract(images, cap=cap, descriptors=descriptors)
    assert ei.value.code == capi.SVO_ERR_CAPACITY and ei.value.needed == counts
    want = [tuple(a[:cap] for a in r[:-1]) + ((r[-1][:cap],) if descriptors else (None,)) for r in full]
    assert [len(r[0]) for r in ei.value.prefix] == [min(k, cap) for k in counts]
    assert_same(ei.value.prefix, want, "surf prefix")


def test_fast_score_plane(ctx):
    import fast_numpy

    host = ctx.fast_detect(list(batch(3)), score=True)
    dev = ctx.fast_detect(on_device(batch(3)), score=True)
    assert_same(dev, host, "fast score")
    for im, (xy, resp, plane) in zip(batch(3), host):
        assert plane.shape == (H, W) and plane.dtype == np.uint8
        assert np.array_equal(plane, fast_numpy.fast_detect(im, 10, True, 0)[2])
    assert host[0][2].any() and not host[1][2].any()
    assert_same([r[:2] for r in host], host_run(ctx, "fast_detect", 3), "fast with and without the plane")
