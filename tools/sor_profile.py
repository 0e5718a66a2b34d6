"""svo_sor_filter_large alone on device inputs: HIP events recorded on the context's stream around the call (which ends
in its own read-back of the counts), median of the repeats.  Clouds: 9216 points at mean_k 200 beside svo_sor_filter
on the same cloud; 50 000, 200 000 and 466 616 (1241 x 376) points sampled like a depth map at mean_k 20 and 200; the
466 616 cloud with and without 1 % outliers through its bounding box.  Prints JSON lines (--out: also written there).
Kernel shares come from one rocprofv3 --kernel-trace --stats run of this script (profiles/README.md)."""
import argparse
import ctypes as C
import json
import pathlib
import statistics
import sys

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from ros_stereo_slam_amd import capi  # noqa: E402
from test_gpu_sor_large import depth_cloud  # noqa: E402
from test_oracle_sor import cloud  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.is_available()
    ctx = capi.Context(0)
    lib = ctx.lib
    stream = torch.cuda.ExternalStream(lib.svo_ctx_stream(ctx._h))
    lines = []

    def timed(fn, label, n, k, outl):
        xyz, col = (cloud(n, seed=1, outliers=int(n * outl)) if label == "test_oracle_sor.cloud"
                    else depth_cloud(n, seed=n, outliers=outl))
        X, Cc = torch.from_numpy(xyz).cuda(), torch.from_numpy(col).cuda()
        xo, co, md = torch.empty_like(X), torch.empty_like(Cc), torch.empty(n, dtype=torch.float32, device="cuda")
        kept, passed = C.c_int(), C.c_int()
        f = getattr(lib, fn)
        torch.cuda.synchronize()

        def call():
            rc = f(ctx._h, capi._ptr(X), capi._ptr(Cc), n, k, C.c_double(0.8), C.c_float(0.0), capi._ptr(xo),
                   capi._ptr(co), C.byref(kept), capi._ptr(md), C.byref(passed), capi.MEM_DEVICE)
            assert rc == 0, lib.svo_last_error()

        for _ in range(3):
            call()
        times = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            call()
            b.record(stream)
            b.synchronize()
            times.append(a.elapsed_time(b))
        rec = {"fn": fn, "cloud": label, "n": n, "mean_k": k, "outliers": outl, "kept": kept.value,
               "ms_median": round(statistics.median(times), 4), "ms_min": round(min(times), 4),
               "ms_max": round(max(times), 4)}
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    timed("svo_sor_filter", "test_oracle_sor.cloud", 9216, 200, 0.025)
    timed("svo_sor_filter_large", "test_oracle_sor.cloud", 9216, 200, 0.025)
    for n in (50000, 200000, 466616):
        for k in (20, 200):
            timed("svo_sor_filter_large", "depth_cloud", n, k, 0.01)
    timed("svo_sor_filter_large", "depth_cloud", 466616, 20, 0.0)
    ctx.close()
    if args.out:
        pathlib.Path(args.out).write_text("".join(json.dumps(r) + "\n" for r in lines))


if __name__ == "__main__":
    main()
