#!/usr/bin/env python3
"""Times one set of pyramid launches ALONE (svo_pyramid_build_many: the 16 left images, with derivative levels, and the 16
right images, without, of a lock-step group step at the bench's image size) on grey frames and on Scene(colour=True) frames:
HIP events on the context's stream, 5 warm-up sets, the median of 20.  Colour frames pay the head launch of a three-channel
build and get nothing for it; grey frames get the one-channel storage.  One JSON line.

    [SVO_LIB=ab/lib_<variant>.so] python tools/pyr_build_profile.py
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
    poses = synth.loop_trajectory(16, **synth.BENCH_LOOP)
    out = {"pyramids": 32, "size": [w, h], "lib": os.environ.get("SVO_LIB", "installed")}
    pyrs = [ctx.pyramid(w, h, 3, want_deriv=k < 16) for k in range(32)]
    for name, colour in (("grey", False), ("colour", True)):
        lefts, rights = synth.stereo_torch(synth.bench_scene(colour=colour), poses, device="cuda", batch=8)
        images = list(lefts) + list(rights)
        torch.cuda.synchronize()
        times = []
        for it in range(25):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            ctx.build_pyramids(pyrs, images)
            e1.record(st)
            ctx.sync()
            e1.synchronize()
            if it >= 5:
                times.append(e0.elapsed_time(e1) * 1e3)
        out[name + "_us_median"] = round(statistics.median(times), 1)
        out[name + "_us_min_max"] = [round(min(times), 1), round(max(times), 1)]
        out[name + "_mono_words"] = sum(p.is_mono() for p in pyrs)
    for p in pyrs:
        p.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
