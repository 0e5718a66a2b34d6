#!/usr/bin/env python3
"""Times svo_ba_window on one GPU and prints one JSON line per measurement.

  workload   4096 points, 8 free poses and the held keyframe, every point seen by every pose, the keyframe's observation in
             stereo, noise 0.3 px, 10 iterations -- the shape a keyframe's window has
  yardstick  the one-pose problem of 4096 points (mono, fx = fy) through svo_ba_window and through svo_ba_3d2d on the same
             data: the one-workgroup kernel is the yardstick, the new path is not

Wall-clock of the synchronous host call (staging, launches, the host's waits and the read-back included): the median and the
spread of --repeat calls after --warmup.  The host waits once for the first look and once per trial; the count is reported.
Per-kernel times are not taken here (use a kernel trace on this script for them).

    python tools/ba_window_profile.py [--repeat 30] [--warmup 5] [--out profiles/ba_window_profile.jsonl]
"""
import argparse
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def timed(fn, repeat, warmup):
    for _ in range(warmup):
        out = fn()
    ts = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts = np.array(ts)
    return out, dict(median_ms=float(np.median(ts)), min_ms=float(ts.min()), p90_ms=float(np.percentile(ts, 90)), repeat=repeat)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch

    torch.cuda.is_available()
    import ba_window_fixtures as F
    from ba_fixtures import K4, problem
    from ros_stereo_slam_amd import capi

    ctx = capi.Context(0)
    lines = []
    w = F.window(n=4096, n_poses=9, seed=1, pattern="all", noise=0.3)
    prm = dict(fx=F.K4[0], fy=F.K4[1], cx=F.K4[2], cy=F.K4[3], bf=F.BF, iterations=10)
    (P, X, chi, info), t = timed(lambda: ctx.ba_window(*F.args(w), params=prm), a.repeat, a.warmup)
    lines.append(dict(what="window 4096 points, 8 free + 1 held poses, 10 iterations", observations=info["observations"],
                      trials=info["trials"], host_waits=1 + info["trials"], chi2_before=info["chi2_before"],
                      chi2_after=info["chi2_after"], per_trial_ms=t["median_ms"] / max(info["trials"], 1), **t))
    uv, X1, R0, t0, _ = problem(4096, 2)
    uvr = np.c_[uv, np.full(len(uv), np.nan, np.float32)].astype(np.float32)
    one = dict(fx=K4[0], fy=K4[0], cx=K4[2], cy=K4[3], iterations=10)
    (_, _, _, iw), tw = timed(lambda: ctx.ba_window(np.r_[R0.ravel(), t0][None], [0], X1, np.arange(4097), np.zeros(4096, np.int32),
                                                    uvr, params=one), a.repeat, a.warmup)
    (_, _, _, i1), t1 = timed(lambda: ctx.ba_3d2d(uv, X1, K4, R0, t0, iterations=10), a.repeat, a.warmup)
    lines.append(dict(what="one pose, 4096 points, 10 iterations: svo_ba_window", trials=iw["trials"], host_waits=1 + iw["trials"], **tw))
    lines.append(dict(what="one pose, 4096 points, 10 iterations: svo_ba_3d2d (one launch)", trials=i1["trials"], host_waits=1, **t1))
    text = "\n".join(json.dumps(l) for l in lines)
    print(text)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
