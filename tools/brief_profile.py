"""svo_brief_describe_batch alone: 2 images of 1241 x 376 grey with 20000 key points each (all inside the border), device inputs,
32 and 64 bytes -- 3 warm-up calls, then 20 timed ones: the context's kernel timers (integral; filter + descriptors) and the wall
time of the Python call, one JSON line per descriptor length.  Run it under `rocprofv3 --kernel-trace --stats` for the per-kernel
times of profiles/brief_kernel_stats.csv.

    python tools/brief_profile.py"""
import json
import pathlib
import sys
import time

import numpy as np
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))
from ros_stereo_slam_amd import capi, synth

torch.cuda.is_available()
ctx = capi.Context(0)
poses = synth.corridor_trajectory(2, step=0.5)
imgs = [np.ascontiguousarray(synth.Scene().render(R, t, channels=1)[0].reshape(376, 1241)) for R, t in poses]
rng = np.random.default_rng(0)
pts = [rng.uniform([28, 28], [1241 - 29, 376 - 29], (20000, 2)).astype(np.float32) for _ in range(2)]
d_imgs = [torch.from_numpy(im).cuda() for im in imgs]
d_pts = [torch.from_numpy(p).cuda() for p in pts]
for nbytes in (32, 64):
    for _ in range(3):
        out = ctx.brief_describe(d_imgs, d_pts, nbytes)
    ctx.enable_kernel_timing(True)
    ctx.reset_kernel_time()
    wall = []
    for _ in range(20):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = ctx.brief_describe(d_imgs, d_pts, nbytes)
        wall.append((time.perf_counter() - t0) * 1e3)
    ti, ni = ctx.kernel_time(capi.K_BRIEF_INTEGRAL)
    td, nd = ctx.kernel_time(capi.K_BRIEF_DESCRIBE)
    ctx.enable_kernel_timing(False)
    print(json.dumps({"case": "2 x 20000 key points, 1241 x 376 grey, device inputs", "bytes": nbytes, "kept": [len(o[1]) for o in out],
                      "integral_ms_per_call": ti / ni, "filter_describe_ms_per_call": td / nd,
                      "python_call_ms_median": float(np.median(wall)), "python_call_ms_min": float(np.min(wall))}))
ctx.close()
