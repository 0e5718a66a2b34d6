"""svo_surf_extract_batch alone: 2 images of 1241 x 376 grey, device inputs, hessian thresholds 500 and 100 -- 3 warm-up calls, then
20 timed ones: the wall time of the Python call, one JSON line per threshold; then the numpy restatement (tests/surf_numpy.py) on
the first image at 500 as the CPU figure, and svo_surf_describe on the 32 largest and the 32 smallest key points for the
descriptor's time per key point at both ends of the scale range.  Run it under `rocprofv3 --kernel-trace --stats` for the
per-kernel times of profiles/surf_kernel_stats.csv.

    python tools/surf_profile.py [--no-cpu]"""
import json
import pathlib
import sys
import time

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from ros_stereo_slam_amd import capi, synth

torch.cuda.is_available()
ctx = capi.Context(0)
poses = synth.corridor_trajectory(2, step=0.5)
imgs = [np.ascontiguousarray(synth.Scene().render(R, t, channels=1)[0].reshape(376, 1241)) for R, t in poses]
d_imgs = [torch.from_numpy(im).cuda() for im in imgs]
for thr in (500, 100):
    prm = dict(hessian_threshold=thr)
    for _ in range(3):
        out = ctx.surf_extract(d_imgs, prm, cap=8192)
    wall = []
    for _ in range(20):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = ctx.surf_extract(d_imgs, prm, cap=8192)
        wall.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"case": "2 x 1241 x 376 grey, device inputs", "hessian_threshold": thr, "key_points": [len(o[0]) for o in out],
                      "largest_size": [float(o[1].max()) for o in out], "python_call_ms_median": float(np.median(wall)),
                      "python_call_ms_min": float(np.min(wall))}))
xy, size = out[0][0], out[0][1]
order = np.argsort(size, kind="stable")
for name, sel in (("smallest", order[:32]), ("largest", order[-32:])):
    for _ in range(2):
        ctx.surf_describe(imgs[0], xy[sel], size[sel])
    t0 = time.perf_counter()
    for _ in range(10):
        ctx.surf_describe(imgs[0], xy[sel], size[sel])
    ms = (time.perf_counter() - t0) * 100
    print(json.dumps({"case": f"svo_surf_describe, the 32 {name} key points (host call, integral image included)",
                      "sizes": [float(size[sel].min()), float(size[sel].max())], "call_ms": ms}))
if "--no-cpu" not in sys.argv:
    import surf_numpy as sn

    t0 = time.perf_counter()
    ref = sn.extract(imgs[0], hessian_threshold=500)
    print(json.dumps({"case": "numpy restatement, image 0, threshold 500", "key_points": len(ref["xy"]),
                      "wall_s": time.perf_counter() - t0}))
ctx.close()
