"""csrc/scan_ops.hip.h, the block prefix scan under every ordered compaction of the library, driven directly through
svo_selftest_scan: one workgroup runs block_scan_counts over n elements, for each of the three (workgroup size, element type)
pairs the kernels use.  The sizes stand on both sides of every seam of the scan -- a lane (1), a wave (63 / 64 / 65), a workgroup
of 256 (255 / 256 / 257) and of 1024 (1023 / 1024 / 1025), and several chunks with a carry (4097, which is also the coverage of
the "more than one item per thread" paths of orb.hip's strip scan and sift.hip's offsets scan: no image small enough for a test
reaches them, and what they add to the block scan is a serial loop per thread).  Integer sums: numpy.cumsum, exactly equal."""
import numpy as np
import pytest

from ros_stereo_slam_amd import capi

pytestmark = pytest.mark.gpu
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097]
KINDS = sorted(capi.SCAN_KINDS)


def run_scan(ctx, kind, values, in_place=False):
    """-> (offsets, total) of the device scan of `values`; the output starts as a sentinel that no prefix sum of the tests equals"""
    import torch

    dt = np.dtype(capi.SCAN_KINDS[kind][1])
    n = len(values)
    dev = torch.device("cuda", 0)
    # torch has no unsigned 32 / 64-bit arithmetic, but the bytes are all this needs
    carrier = {4: torch.int32, 8: torch.int64}[dt.itemsize]
    signed = np.dtype(f"int{8 * dt.itemsize}")
    host_in = np.ascontiguousarray(values, dt)
    d_in = torch.from_numpy(np.concatenate([host_in, np.zeros(1, dt)]).view(signed)).to(dev)   # never empty
    d_out = d_in if in_place else torch.full((n + 1,), -7, dtype=carrier, device=dev)
    d_total = torch.full((1,), -7, dtype=carrier, device=dev)
    torch.cuda.synchronize()
    ctx.selftest_scan(kind, d_in, n, d_out, d_total)
    out = d_out.cpu().numpy().view(dt)
    assert out[n] == (0 if in_place else np.array(-7, signed).astype(dt)), "written past n"
    if not in_place:
        assert np.array_equal(d_in.cpu().numpy().view(dt)[:n], host_in), "the input changed"
    return out[:n].copy(), d_total.cpu().numpy().view(dt)[0]


def expect(values, dt):
    v = np.asarray(values, dt)
    incl = np.cumsum(v, dtype=dt)
    return incl - v, (incl[-1] if len(v) else dt.type(0))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_scan_equals_cumsum(ctx, kind, n):
    dt = np.dtype(capi.SCAN_KINDS[kind][1])
    rng = np.random.default_rng(1000 * KINDS.index(kind) + n)
    for name, values in (("random", rng.integers(0, 4, n)), ("zeros", np.zeros(n, np.int64)), ("ones", np.ones(n, np.int64))):
        off, total = run_scan(ctx, kind, values.astype(dt))
        e_off, e_total = expect(values, dt)
        assert off.dtype == dt and np.array_equal(off, e_off), (kind, n, name)
        assert total == e_total, (kind, n, name, total, e_total)


@pytest.mark.parametrize("kind", KINDS)
def test_scan_in_place(ctx, kind):
    dt = np.dtype(capi.SCAN_KINDS[kind][1])
    values = np.random.default_rng(7).integers(0, 4, 4097).astype(dt)
    off, total = run_scan(ctx, kind, values, in_place=True)
    e_off, e_total = expect(values, dt)
    assert np.array_equal(off, e_off) and total == e_total


def test_64_bit_carry_passes_2_to_the_32(ctx):
    """1025 entries of 2^30: the wave totals, the block total and the carry into the second chunk all pass 2^32 -- the sums
    match.hip's radius_scan_kernel saturates only AFTER they are formed in 64 bits"""
    values = np.full(1025, 1 << 30, np.uint64)
    off, total = run_scan(ctx, "1024_u64", values)
    assert np.array_equal(off, np.arange(1025, dtype=np.uint64) << np.uint64(30))
    assert int(total) == 1025 << 30 and int(total) > 1 << 32 and int(off[1024]) == 1 << 40
