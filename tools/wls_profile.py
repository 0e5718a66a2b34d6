"""The disparity WLS filter at KITTI's 1241 x 376 with the reference's parameters (matcher 1 / 96 / 7, lambda 400, sigma
0.4), batch 1 and 16: svo_sgbm_compute alone, svo_sgbm_wls_compute (both matchers + the filter) and svo_wls_filter alone
(on the maps the chain left).  Device inputs, HIP events recorded on the context's stream around the asynchronous call,
3 warm-up calls, median of the repeats.  Prints one JSON line per batch size.

    python tools/wls_profile.py [--reps 20] [--batches 1,16]"""
import argparse
import ctypes as C
import json
import pathlib
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))
from ros_stereo_slam_amd import capi, synth


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batches", default="1,16")
    args = ap.parse_args()
    torch.cuda.is_available()
    ctx = capi.Context(0)
    lib = ctx.lib
    stream = torch.cuda.ExternalStream(lib.svo_ctx_stream(ctx._h))
    w, h = synth.KITTI_SIZE
    sp = capi.sgbm_params()
    wp = capi.wls_params(sp, lambda_=400.0, sigma_color=0.4)

    def timed(call):
        for _ in range(3):
            call()
        lib.svo_ctx_sync(ctx._h)
        times = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            call()
            b.record(stream)
            b.synchronize()
            times.append(a.elapsed_time(b))
        return statistics.median(times), min(times), max(times)

    for n in [int(b) for b in args.batches.split(",")]:
        pairs = [synth.textured_pair(w, h, 3, shift=(7 + k, 0), seed=100 + k) for k in range(n)]
        L = torch.from_numpy(np.stack([p[1] for p in pairs])).cuda()
        R = torch.from_numpy(np.stack([p[0] for p in pairs])).cuda()
        mk = lambda dt: torch.empty((n, h, w), dtype=dt, device="cuda")
        raw, filt, dl, dr, conf, filt2, conf2 = (mk(torch.int16), mk(torch.int16), mk(torch.int16), mk(torch.int16),
                                                 mk(torch.float32), mk(torch.int16), mk(torch.float32))
        grey = torch.empty((n, h, w), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

        def ok(rc):
            assert rc == 0, lib.svo_last_error()

        def sgbm():
            ok(lib.svo_sgbm_compute(ctx._h, C.byref(sp), capi._ptr(L), capi._ptr(R), w, h, 3, n, capi._ptr(raw), capi.MEM_DEVICE))

        def chain():
            ok(lib.svo_sgbm_wls_compute(ctx._h, C.byref(sp), C.byref(wp), capi._ptr(L), capi._ptr(R), w, h, 3, n, capi._ptr(filt),
                                        capi._ptr(dl), capi._ptr(dr), capi._ptr(conf), capi.MEM_DEVICE))

        def filter_only():
            ok(lib.svo_wls_filter(ctx._h, C.byref(wp), capi._ptr(dl), capi._ptr(dr), capi._ptr(grey), w, h, 1, n,
                                  capi._ptr(filt2), capi._ptr(conf2), capi.MEM_DEVICE))

        t_sgbm = timed(sgbm)
        t_chain = timed(chain)
        # the guide of the filter alone: the grey left images, converted once outside the timed calls
        lefts = np.stack([p[1] for p in pairs]).astype(np.int64)
        grey.copy_(torch.from_numpy(((1868 * lefts[..., 0] + 9617 * lefts[..., 1] + 4899 * lefts[..., 2] + 8192) >> 14)
                                    .astype(np.uint8)).cuda())
        torch.cuda.synchronize()
        t_filter = timed(filter_only)
        lib.svo_ctx_sync(ctx._h)
        same = bool(torch.equal(filt, filt2) and torch.equal(conf, conf2) and torch.equal(raw, dl))
        x0, y0 = wp.roi_left, wp.roi_top
        rw, rh = w - wp.roi_left - wp.roi_right, h - wp.roi_top - wp.roi_bottom
        frac = float((conf[:, y0:y0 + rh, x0:x0 + rw] > 0).float().mean())
        rec = {"batch": n, "reps": args.reps, "roi": [rw, rh], "filter_alone_equals_chain": same,
               "confidence_positive_fraction_of_roi": round(frac, 3)}
        for name, (med, lo, hi) in (("sgbm", t_sgbm), ("sgbm_wls", t_chain), ("wls_filter", t_filter)):
            rec[name + "_ms_per_call"] = round(med, 4)
            rec[name + "_ms_per_pair"] = round(med / n, 4)
            rec[name + "_ms_min_max"] = [round(lo, 4), round(hi, 4)]
        print(json.dumps(rec), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
