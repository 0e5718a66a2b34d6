"""svo_star_detect_batch beside svo_fast_detect_batch and svo_surf_extract_batch (detect only) on the same device-resident 1241 x 376
images, batches of 1 and 16: a host clock around each call (every one ends in its wait for the counts), the three detectors taking
turns round by round, median over the rounds after warm-up.  Prints JSON lines (--out: also written there).  The per-kernel split
comes from running this script under a kernel trace in a run of its own (--brief: one round, Star only)."""
import argparse
import ctypes as C
import json
import pathlib
import statistics
import sys
import time

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from ros_stereo_slam_amd import capi, synth  # noqa: E402

SIZE, K4 = (1241, 376), (718.856, 718.856, 607.1928, 185.2157)


def frames(n):
    """n different images of one size: two rendered views, the rest shifted copies of them."""
    base = []
    for k in range(2):
        R, t = synth.corridor_trajectory(k + 1, step=0.5)[k]
        base.append(np.ascontiguousarray(synth.Scene().render(R, t, K=K4, size=SIZE, channels=3)[0]))
    return [np.ascontiguousarray(np.roll(base[k & 1], (3 * (k >> 1), 5 * (k >> 1)), axis=(0, 1))) for k in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--brief", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rounds, warm = (1, 1) if args.brief else (args.rounds, 5)
    torch.cuda.is_available()   # torch's HIP runtime loads first, so that one copy serves torch and the library
    ctx = capi.Context(0)
    lib = ctx.lib
    vp, ci = C.c_void_p, C.c_int
    lib.svo_star_detect_batch.argtypes = [vp, vp, ci, ci, ci, ci, vp, ci, vp, vp, vp, vp, ci]
    lib.svo_fast_detect_batch.argtypes = [vp, vp, ci, ci, ci, ci, vp, ci, vp, vp, vp, vp, ci]
    lib.svo_surf_extract_batch.argtypes = [vp, vp, ci, ci, ci, ci, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, ci]
    cap = 100000

    def job(fn, imgs, prm, n_cols):
        """A call of detector `fn` on device images -> (record, call, counts, the device arrays the call uses: kept alive here)."""
        nimg = len(imgs)
        h, w = imgs[0].shape[:2]
        c = 1 if imgs[0].ndim == 2 else imgs[0].shape[2]
        dev = [torch.from_numpy(im).cuda() for im in imgs]
        out = torch.zeros(nimg * cap * (n_cols + 1), dtype=torch.float32, device="cuda")
        n = (C.c_int * nimg)()
        ptrs = (C.c_void_p * nimg)(*[d.data_ptr() for d in dev])
        cols = [C.c_void_p(out.data_ptr() + 4 * nimg * cap * k) for k in (0, *range(2, n_cols + 1))]
        torch.cuda.synchronize()
        if fn == "svo_star_detect_batch":
            call = lambda: lib.svo_star_detect_batch(ctx._h, ptrs, nimg, w, h, c, C.byref(prm), cap, *cols, n, capi.MEM_DEVICE)
        elif fn == "svo_fast_detect_batch":
            call = lambda: lib.svo_fast_detect_batch(ctx._h, ptrs, nimg, w, h, c, C.byref(prm), cap, *cols, None, n, capi.MEM_DEVICE)
        else:
            call = lambda: lib.svo_surf_extract_batch(ctx._h, ptrs, nimg, w, h, c, C.byref(prm), cap, *cols, None, n, capi.MEM_DEVICE)
        rec = {"fn": fn, "images": nimg, "size": f"{w}x{h}x{c}"}
        return rec, call, (lambda: list(n[:nimg])), (dev, out)

    bgr = frames(16)
    lines = []
    for nimg in (1, 16):
        jobs = [job("svo_star_detect_batch", bgr[:nimg], capi.star_params(), 3)]
        if not args.brief:
            jobs.append(job("svo_fast_detect_batch", bgr[:nimg], capi.fast_params(threshold=20), 2))
            jobs.append(job("svo_surf_extract_batch", bgr[:nimg], capi.surf_params(hessian_threshold=500.0), 6))
        times = [[] for _ in jobs]
        for r in range(warm + rounds):
            for k, (_, call, _, _) in enumerate(jobs):      # taking turns: a drift of the clock or the machine hits all alike
                t0 = time.perf_counter()
                rc = call()
                dt = (time.perf_counter() - t0) * 1e3
                assert rc == 0, lib.svo_last_error()
                if r >= warm:
                    times[k].append(dt)
        for (rec, _, counts, _), t in zip(jobs, times):
            rec.update(keypoints=counts(), rounds=rounds, ms_median=round(statistics.median(t), 4), ms_min=round(min(t), 4),
                       ms_max=round(max(t), 4), ms_median_per_image=round(statistics.median(t) / rec["images"], 4))
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    ctx.close()
    if args.out:
        pathlib.Path(args.out).write_text("".join(json.dumps(r) + "\n" for r in lines))


if __name__ == "__main__":
    main()
