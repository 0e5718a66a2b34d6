"""Time svo_rectify_pairs on one MI355X: 16 pairs at 752 x 480 grey and at 1241 x 376 BGR, device memory, a host clock around a
window of back-to-back calls that ends in a device synchronise.  The calls rotate through 16 sets of source and output buffers,
more than the Infinity Cache holds, so the images move through HBM; the time on one set, which stays cached, is printed too.
Beside them the floor from the algorithmic bytes (6 + 2 c) w h per image (6 map bytes read, c source bytes read about once, c bytes written per pixel; the map is
charged per image although one pair serves all 16, so the floor is generous to the kernel's share) at the HBM
rate a float4 copy reaches on this part, 6.29 TB/s.  Usage: python tools/rectify_profile.py [--reps 2000]"""
import argparse
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
HBM_BYTES_PER_S = 6.29e12
SETS = 16   # buffer sets the timed calls rotate through


def main():
    import torch

    import rectify_fixtures as rf
    from ros_stereo_slam_amd import capi

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2000)
    args = ap.parse_args()
    ctx = capi.Context(0)
    K1, D1, K2, D2, _, R, T = rf.RIGS["euroc"]
    for (w, h), c in (((752, 480), 1), ((1241, 376), 3)):
        s = w / 752.0
        S = np.diag([s, h / 480.0, 1.0])
        rect = capi.stereo_rectify(S @ K1, D1, S @ K2, D2, (w, h), R, T)
        ml, mr = ctx.rectify_map(S @ K1, D1, rect.R1, rect.P1, (w, h)), ctx.rectify_map(S @ K2, D2, rect.R2, rect.P2, (w, h))
        g = torch.Generator().manual_seed(1)
        shape = (16, h, w, c) if c == 3 else (16, h, w)
        # SETS buffer sets taken in turn, more than the 256 MB Infinity Cache holds, so that sources and outputs come from and go to
        # HBM; the two maps are one pair for every call, as in use, and stay cached
        sets = []
        for _ in range(SETS):
            L, Rr = (torch.randint(0, 256, shape, dtype=torch.uint8, generator=g).cuda() for _ in range(2))
            sets.append((L, Rr, torch.empty_like(L), torch.empty_like(Rr)))
        assert SETS * 4 * sets[0][0].numel() > 256 << 20

        def call(k):
            L, Rr, ol, orr = sets[k % SETS]
            capi._check(ctx.lib.svo_rectify_pairs(ctx._h, ml._h, mr._h, capi._ptr(L), capi._ptr(Rr), 16, c, 0, capi._ptr(ol), capi._ptr(orr),
                                                  capi.MEM_DEVICE))

        for k in range(2 * SETS):
            call(k)
        ctx.sync()
        t0 = time.perf_counter()
        for k in range(args.reps):
            call(k)
        ctx.sync()
        us = (time.perf_counter() - t0) * 1e6 / args.reps
        one = sets[0]
        t0 = time.perf_counter()
        for k in range(args.reps):
            capi._check(ctx.lib.svo_rectify_pairs(ctx._h, ml._h, mr._h, capi._ptr(one[0]), capi._ptr(one[1]), 16, c, 0, capi._ptr(one[2]),
                                                  capi._ptr(one[3]), capi.MEM_DEVICE))
        ctx.sync()
        hot_us = (time.perf_counter() - t0) * 1e6 / args.reps
        floor_us = 32 * (6 + 2 * c) * w * h / HBM_BYTES_PER_S * 1e6
        print(f"svo_rectify_pairs 16 pairs {w} x {h} x {c}: {us:8.1f} us per call, byte floor {floor_us:6.1f} us at 6.29 TB/s, "
              f"{floor_us / us * 100:5.1f} % of the floor's rate; the same buffers every call (cache-resident): {hot_us:6.1f} us")
        del sets
        ml.close()
        mr.close()
    ctx.close()


if __name__ == "__main__":
    main()
