"""svo_find_homography alone on device inputs, and svo_find_essential at the same sizes in the same run: HIP events
recorded on the context's stream around the call, median of the repeats.  One problem at n = 500 / 2 000 / 8 000 pairs
with inlier ratios 0.9 / 0.5 / 0.3 (0.5 px noise), and a batch of 16 problems of 2 000 pairs at 0.5; svo_homography_pose on
the 2 000-pair problem.  The homography's pairs lie on one plane, the essential matrix's in a general scene (each
estimator on data it is made for).  Prints JSON lines (--out: also written there)."""
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
from test_gpu_essential import pixel_problem  # noqa: E402
from test_homography_numpy import K4, plane_problem  # noqa: E402


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

    def timed(label, probs, fn_name):
        a = torch.from_numpy(np.concatenate([p[0] for p in probs])).cuda()
        b = torch.from_numpy(np.concatenate([p[1] for p in probs])).cuda()
        nprob = len(probs)
        offsets = np.ascontiguousarray(np.concatenate([[0], np.cumsum([len(p[0]) for p in probs])]), np.int32)
        K = np.ascontiguousarray(np.tile(np.asarray(K4, np.float64), nprob))
        total = int(offsets[-1])
        mask = torch.empty(total, dtype=torch.uint8, device="cuda")
        M = torch.zeros((nprob, 90), dtype=torch.float64, device="cuda")
        ints = torch.zeros((3, nprob), dtype=torch.int32, device="cuda")
        R = torch.zeros((nprob, 9), dtype=torch.float64, device="cuda")
        t = torch.zeros((nprob, 3), dtype=torch.float64, device="cuda")
        nrm = torch.zeros((nprob, 3), dtype=torch.float64, device="cuda")
        good4 = torch.zeros((nprob, 4), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

        def call(name):
            if name == "svo_find_essential":
                rc = lib.svo_find_essential(ctx._h, capi._ptr(a), capi._ptr(b), capi._ptr(offsets), nprob, capi._ptr(K),
                                            C.c_double(1.0), C.c_double(0.99), 1000, C.c_uint64(7), capi._ptr(mask), capi._ptr(M),
                                            capi._ptr(ints[0]), capi._ptr(ints[1]), capi._ptr(ints[2]), capi.MEM_DEVICE)
            elif name == "svo_find_homography":
                rc = lib.svo_find_homography(ctx._h, capi._ptr(a), capi._ptr(b), capi._ptr(offsets), nprob, C.c_double(3.0),
                                             C.c_double(0.995), 2000, C.c_uint64(7), capi._ptr(mask), capi._ptr(M), capi._ptr(ints[1]),
                                             capi._ptr(ints[2]), capi.MEM_DEVICE)
            else:
                rc = lib.svo_homography_pose(ctx._h, capi._ptr(M), capi._ptr(a), capi._ptr(b), capi._ptr(offsets), nprob, capi._ptr(K),
                                             C.c_double(50.0), None, capi._ptr(R), capi._ptr(t), capi._ptr(nrm),
                                             capi._ptr(good4), capi.MEM_DEVICE)
            assert rc == 0, lib.svo_last_error()

        if fn_name == "svo_homography_pose":
            call("svo_find_homography")
        for _ in range(3):
            call(fn_name)
        times = []
        for _ in range(args.reps):
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record(stream)
            call(fn_name)
            ev1.record(stream)
            ev1.synchronize()
            times.append(ev0.elapsed_time(ev1))
        it = ints.cpu().numpy()
        rec = {"fn": fn_name, "case": label, "problems": nprob, "pairs": total, "iters_run": it[2].tolist()[:4],
               "inliers": it[1].tolist()[:4], "ms_median": round(statistics.median(times), 4), "ms_min": round(min(times), 4),
               "ms_max": round(max(times), 4)}
        if it[2][0] > 0:
            rec["us_per_iteration"] = round(1e3 * rec["ms_median"] / float(it[2].max()), 3)
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    for n in (500, 2000, 8000):
        for ratio in (0.9, 0.5, 0.3):
            seed = n + int(ratio * 10)
            timed(f"n={n} inliers={ratio}", [plane_problem(n, 1 - ratio, seed, noise=0.5)], "svo_find_homography")
            timed(f"n={n} inliers={ratio}", [pixel_problem(n, 1 - ratio, seed=seed, noise=0.5)], "svo_find_essential")
    timed("batch 16 x n=2000 inliers=0.5", [plane_problem(2000, 0.5, 900 + k, noise=0.5) for k in range(16)], "svo_find_homography")
    timed("batch 16 x n=2000 inliers=0.5", [pixel_problem(2000, 0.5, seed=900 + k, noise=0.5) for k in range(16)], "svo_find_essential")
    timed("n=2000 inliers=0.5", [plane_problem(2000, 0.5, 2005, noise=0.5)], "svo_homography_pose")
    ctx.close()
    if args.out:
        pathlib.Path(args.out).write_text("".join(json.dumps(r) + "\n" for r in lines))


if __name__ == "__main__":
    main()
