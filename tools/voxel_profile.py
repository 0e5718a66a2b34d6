"""svo_voxel_downsample on the rendered dense cloud of DESIGN.md section 10 (the synthetic corridor through svo_sgbm_compute and
svo_stereo_reproject with the metric Q, z up to 80 m), device inputs: leaves 0.05 and 0.2 and one leaf that puts the whole cloud
into a single voxel.  Beside each: svo_sor_filter_large(20, 0.8) on the full cloud and on the thinned one.  Every call ends in its
own read-back of the counts, so a host clock around it measures the device work and the waits; warm-up calls first, median of the
repeats.  The floor printed with them is the cloud's bytes (points and colours, read once and the thinned cloud written once) over
the measured HBM copy rate.  Prints text lines (--out: also written there)."""
import argparse
import pathlib
import statistics
import sys
import time

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from ros_stereo_slam_amd import capi, synth  # noqa: E402

HBM_BYTES_PER_S = 6.29e12   # MI355X, measured float4 copy


def dense_cloud(ctx):
    left, right, _ = synth.Scene().stereo(np.eye(3), np.zeros(3), channels=3)
    disp = ctx.sgbm(left, right)
    fx, fy, cx, cy = synth.KITTI_K
    Q = capi.stereo_rectify_q(fx, fy, cx, cy, -0.5707, left.shape[1], left.shape[0])
    return ctx.stereo_reproject(disp, left, Q, disp_scale=1 / 16, z_max=80.0)


def median_ms(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("voxel_profile needs the GPU: there is no CPU path to time")
    ctx = capi.Context(0)
    xyz, bgr = dense_cloud(ctx)
    n = len(xyz)
    X, B = torch.from_numpy(xyz).cuda(), torch.from_numpy(bgr).cuda()
    lines = [f"cloud: {n} points with colours, {n * 24} bytes"]
    full = median_ms(lambda: ctx.sor_filter_large(X, B, mean_k=20, stddev_mul=0.8), args.reps)
    lines.append(f"svo_sor_filter_large(20, 0.8) on the full cloud: median {full[0]:.3f} ms (min {full[1]:.3f}, max {full[2]:.3f})")
    extent = float(np.abs(xyz[np.isfinite(xyz).all(1)]).max())
    for label, leaf in (("0.05", 0.05), ("0.2", 0.2), ("one voxel", 4.0 * extent + 1.0)):
        xo, co = ctx.voxel_downsample(X, leaf, B)
        k = len(xo)
        t = median_ms(lambda: ctx.voxel_downsample(X, leaf, B), args.reps)
        floor_ms = (n * 24 + k * 24) / HBM_BYTES_PER_S * 1e3
        lines.append(f"leaf {label}: {n} -> {k} points, svo_voxel_downsample median {t[0]:.3f} ms (min {t[1]:.3f}, max {t[2]:.3f}); "
                     f"bytes / HBM rate floor {floor_ms:.4f} ms")
        if k > 1:
            s = median_ms(lambda: ctx.sor_filter_large(xo, co, mean_k=20, stddev_mul=0.8), args.reps)
            lines.append(f"leaf {label}: svo_sor_filter_large(20, 0.8) on the thinned cloud: median {s[0]:.3f} ms "
                         f"(min {s[1]:.3f}, max {s[2]:.3f}); down-sample + filter {t[0] + s[0]:.3f} ms against {full[0]:.3f} ms")
    ctx.close()
    print("\n".join(lines), flush=True)
    if args.out:
        pathlib.Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
