#!/usr/bin/env python3
"""Times the 16-job tracking launch ALONE (svo_lk_track_jobs: frame k -> frame k + 1 of the bench loop, k = 0 .. 15, the
lattice of grid step 10 = the bench's points before ANMS) on grey frames and on Scene(colour=True) frames: HIP events on
the context's stream, 5 warm-up launches, the median of 20.  Grey frames take the tracker's one-channel body, colour frames
must cost what they cost before it existed.  One JSON line.

    [SVO_LIB=ab/lib_<variant>.so] python tools/lk_mono_profile.py
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch

    from ros_stereo_slam_amd import capi, synth

    ctx = capi.Context(0)
    st = torch.cuda.ExternalStream(ctx.stream)
    w, h = synth.KITTI_SIZE
    pts = torch.from_numpy(ctx.grid_keypoints(h, w, 10)).cuda()
    n = pts.shape[0]
    poses = synth.loop_trajectory(17, **synth.BENCH_LOOP)
    out = {"points_per_job": int(n), "jobs": 16, "lib": os.environ.get("SVO_LIB", "installed")}
    for name, colour in (("grey", False), ("colour", True)):
        lefts, _ = synth.stereo_torch(synth.bench_scene(colour=colour), poses, device="cuda", batch=8)
        torch.cuda.synchronize()
        pyrs = [ctx.pyramid(w, h, 3).build(im, capi.MEM_DEVICE) for im in lefts]
        ctx.sync()
        if hasattr(ctx.lib, "svo_pyramid_is_mono"):
            out[name + "_mono_words"] = sum(p.is_mono() for p in pyrs)
        jobs = [(pyrs[k], pyrs[k + 1], pts, torch.empty(n, 2, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda"),
                 None, None, None) for k in range(16)]
        times = []
        for it in range(25):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            ctx.lk_track_jobs(jobs)
            e1.record(st)
            ctx.sync()
            e1.synchronize()
            if it >= 5:
                times.append(e0.elapsed_time(e1) * 1e3)
        out[name + "_us_median"] = round(statistics.median(times), 1)
        out[name + "_us_min_max"] = [round(min(times), 1), round(max(times), 1)]
        out[name + "_tracked"] = int(sum(int(j[4].sum()) for j in jobs))
        for p in pyrs:
            p.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
