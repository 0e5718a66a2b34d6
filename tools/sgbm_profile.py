"""svo_sgbm_compute alone at KITTI's 1241 x 376, D = 96 (the reference's parameters), batch 1 and 16: device
inputs, HIP events recorded on the context's stream around the asynchronous call, median of the repeats.  Prints
JSON lines; with --roofline also the algorithmic bytes of the cost and path kernels over 8 TB/s.  Kernel shares come
from one rocprofv3 --kernel-trace --stats run of this script (profiles/README.md)."""
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
    prm = capi.sgbm_params()
    D, W1 = prm.num_disparities, w - (prm.min_disparity + prm.num_disparities)
    for n in [int(b) for b in args.batches.split(",")]:
        pairs = [synth.textured_pair(w, h, 3, shift=(7 + k, 0), seed=100 + k) for k in range(n)]
        L = torch.from_numpy(np.stack([p[1] for p in pairs])).cuda()
        R = torch.from_numpy(np.stack([p[0] for p in pairs])).cuda()
        out = torch.empty((n, h, w), dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()

        def call():
            rc = lib.svo_sgbm_compute(ctx._h, C.byref(prm), capi._ptr(L), capi._ptr(R), w, h, 3, n, capi._ptr(out),
                                      capi.MEM_DEVICE)
            assert rc == 0, lib.svo_last_error()

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
        ms = statistics.median(times)
        cells = n * h * W1 * D
        # algorithmic bytes: cost = hsum written + read + C written; paths = C read by 4 directions + 4 planes written;
        # WTA = C + 4 planes read
        cost_b, path_b, wta_b = cells * 2 * 3, cells * 2 * 8, cells * 2 * 5
        print(json.dumps({"batch": n, "ms_per_call": round(ms, 4), "ms_per_pair": round(ms / n, 4),
                          "cost_volume_MB_per_pair": round(h * W1 * D * 2 / 1e6, 1),
                          "algorithmic_GB": round((cost_b + path_b + wta_b) / 1e9, 3),
                          "fraction_of_8TBps": round((cost_b + path_b + wta_b) / (ms * 1e-3) / 8e12, 3)}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
