"""svo_bm_compute beside svo_sgbm_compute, each call alone, at KITTI's 1241 x 376 with D = 96 (minDisparity 1), batch 1 and 16, on
the same images in one process: device inputs, HIP events recorded on the context's stream around the asynchronous call, median
of the repeats; with the speckle window at 3000 and again at 0.  Prints JSON lines and writes them to profiles/bm_profile.jsonl
(--out)."""
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
from ros_stereo_slam_amd import capi, synth


def median_ms(lib, ctx, stream, call, reps):
    for _ in range(3):
        call()
    lib.svo_ctx_sync(ctx._h)
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        call()
        b.record(stream)
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batches", default="1,16")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "bm_profile.jsonl"))
    args = ap.parse_args()
    torch.cuda.is_available()
    ctx = capi.Context(0)
    lib = ctx.lib
    stream = torch.cuda.ExternalStream(lib.svo_ctx_stream(ctx._h))
    w, h = synth.KITTI_SIZE
    lines = []
    for n in [int(b) for b in args.batches.split(",")]:
        pairs = [synth.textured_pair(w, h, 3, shift=(7 + k, 0), seed=100 + k) for k in range(n)]
        L = torch.from_numpy(np.stack([p[1] for p in pairs])).cuda()
        R = torch.from_numpy(np.stack([p[0] for p in pairs])).cuda()
        out = torch.empty((n, h, w), dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        for window in (3000, 0):
            bp = capi.bm_params(min_disparity=1, num_disparities=96, speckle_window_size=window, speckle_range=5)
            sp = capi.sgbm_params(speckle_window_size=window)

            def run(fn, prm):
                rc = fn(ctx._h, C.byref(prm), capi._ptr(L), capi._ptr(R), w, h, 3, n, capi._ptr(out), capi.MEM_DEVICE)
                assert rc == 0, lib.svo_last_error()

            bm_ms = median_ms(lib, ctx, stream, lambda: run(lib.svo_bm_compute, bp), args.reps)
            valid = float((out != 0).float().mean().item())
            sgbm_ms = median_ms(lib, ctx, stream, lambda: run(lib.svo_sgbm_compute, sp), args.reps)
            rec = {"batch": n, "speckle_window": window, "w": w, "h": h, "num_disparities": 96, "bm_block": bp.block_size,
                   "bm_ms_per_call": round(bm_ms, 4), "sgbm_ms_per_call": round(sgbm_ms, 4),
                   "bm_ms_per_pair": round(bm_ms / n, 4), "sgbm_ms_per_pair": round(sgbm_ms / n, 4),
                   "sgbm_over_bm": round(sgbm_ms / bm_ms, 2), "bm_valid_share": round(valid, 3)}
            print(json.dumps(rec), flush=True)
            lines.append(json.dumps(rec))
    ctx.close()
    pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
