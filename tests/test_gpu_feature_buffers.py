"""sift.hip, brief.hip and surf.hip stage their images and keep their integral images in buffers of the context that all three share
(svo_ctx::feat_img, ::feat_sum; csrc/feature_batch.hip.h).  A call must not see what an earlier call of another module, image size,
channel count or batch size left there: every call of an interleaved sequence on ONE context returns the bits the same call returns
as the first call of a fresh context.

The images are small (96 x 80 and 72 x 64, so that slot and integral strides change between the calls) and synthetic: seeded noise
plus Gaussian blobs.  On the CPU the restatements find 9 and 20 SIFT key points in the two 96 x 80 images (tests/sift_numpy.py; 7 and
5 of them inside BRIEF's 28-pixel border) and 14 and 10 in the first two grey 72 x 64 images, 18 SURF key points in the 96 x 80 BGR
image (svo_surf_describe keeps all), 7 in the 72 x 64 BGR image and 16, 8 and 15 in the grey ones (tests/surf_numpy.py): no step
passes on empty lists, and each asserts so."""
import numpy as np
import pytest

from ros_stereo_slam_amd import capi

pytestmark = pytest.mark.gpu

A, B = (96, 80), (72, 64)


def blobs(size, c, seed):
    w, h = size
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[:h, :w].astype(np.float64)
    img = 110 + 12 * rng.standard_normal((h, w))
    for _ in range(14):
        cx, cy = rng.uniform(0.2 * w, 0.8 * w), rng.uniform(0.25 * h, 0.75 * h)
        s, a = rng.uniform(1.5, 5.0), rng.choice([-1.0, 1.0]) * rng.uniform(60, 110)
        img += a * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * s * s))
    img = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    if c == 1:
        return img
    return np.ascontiguousarray(np.stack([img, np.roll(img, 1, 1), np.roll(img, 1, 0)], axis=2))


def flat(result):
    """every array of a nested result as (dtype, shape, bytes); None stays None"""
    if result is None:
        return [None]
    if isinstance(result, np.ndarray):
        return [(str(result.dtype), result.shape, result.tobytes())]
    return [leaf for part in result for leaf in flat(part)]


def fresh(call):
    c = capi.Context(0)
    try:
        return call(c)
    finally:
        c.close()


def test_interleaved_calls_on_one_context_equal_first_calls_on_fresh_contexts():
    import torch

    a1 = [blobs(A, 1, 1), blobs(A, 1, 2)]
    a3, b3 = blobs(A, 3, 1), blobs(B, 3, 3)
    b1 = [blobs(B, 1, s) for s in (4, 5, 6)]
    b1_dev = [torch.from_numpy(im).cuda() for im in b1[:2]]
    # three grey device images inside one allocation, unevenly spaced with other bytes between them: svo_surf_extract_batch gathers
    # them into the shared image buffer (surf_prepare), where steps 1 ... 5 staged host images
    px = B[0] * B[1]
    offs = [0, px + 64, 2 * px + 256]
    pool = torch.full((3 * px + 512,), 255, dtype=torch.uint8, device="cuda")
    for off, im in zip(offs, b1):
        pool[off:off + px] = torch.from_numpy(im).cuda().reshape(-1)
    scattered = [pool[off:off + px].view(B[1], B[0]) for off in offs]
    assert offs[2] - offs[0] != 2 * (offs[1] - offs[0])

    sift_a = fresh(lambda c: c.sift_extract(a1, cap=512))
    kp_a = [r[0] for r in sift_a]
    surf_a3 = fresh(lambda c: c.surf_extract([a3], cap=512))[0]
    steps = [
        ("1 sift_extract, host, 2 x A grey", lambda c: c.sift_extract(a1, cap=512)),
        ("2 brief_describe, host, 2 x A grey", lambda c: c.brief_describe(a1, kp_a)),
        ("3 surf_extract, host, 1 x B BGR", lambda c: c.surf_extract([b3], cap=512)),
        ("4 brief_describe again", lambda c: c.brief_describe(a1, kp_a)),
        ("5 surf_describe, host, A BGR", lambda c: c.surf_describe(a3, surf_a3[0], surf_a3[1])),
        ("6 sift_extract, device, 2 x B grey", lambda c: c.sift_extract(b1_dev, cap=512)),
        ("7 surf_extract, device, 3 x B grey unevenly spaced", lambda c: c.surf_extract(scattered, cap=512)),
    ]
    first = [sift_a] + [fresh(call) for _, call in steps[1:]]
    for r in first[0] + first[5]:
        assert len(r[0]) > 0, "SIFT found no key point"
    for r in first[1] + first[3]:
        assert len(r[0]) > 0, "BRIEF kept no key point"
    for r in first[2] + first[6]:
        assert len(r[0]) > 0, "SURF found no key point"
    assert len(surf_a3[0]) > 0 and first[4][2].any(), "svo_surf_describe kept no key point"
    # the gathered batch is the batch of the same images from host memory
    assert flat(first[6]) == flat(fresh(lambda c: c.surf_extract(b1, cap=512)))

    ctx = capi.Context(0)
    try:
        for (name, call), ref in zip(steps, first):
            assert flat(call(ctx)) == flat(ref), f"step {name} differs from the same call on a fresh context"
    finally:
        ctx.close()
