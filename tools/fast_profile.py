"""svo_fast_detect_batch and svo_fast_anms_batch alone on device inputs, with svo_orb_extract_batch on the same images beside them:
HIP events recorded on the context's stream around each call (which includes its wait for the counts), median of the repeats after
warm-up.  1241 x 376 grey and BGR, thresholds 1 and 20, batches of 1 and 16, ANMS with keep 4096.  Prints JSON lines (--out: also
written there).  Per-kernel times (fast_score_kernel against the extractor's cv_blur_corners) come from running this script under a
kernel trace in a run of its own (--brief: one repeat of each case, for that)."""
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
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--brief", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    reps, warm = (1, 1) if args.brief else (args.reps, 5)
    torch.cuda.is_available()
    ctx = capi.Context(0)
    lib = ctx.lib
    stream = torch.cuda.ExternalStream(lib.svo_ctx_stream(ctx._h))
    vp, ci = C.c_void_p, C.c_int
    lib.svo_fast_detect_batch.argtypes = [vp, vp, ci, ci, ci, ci, vp, ci, vp, vp, vp, vp, ci]
    lib.svo_fast_anms_batch.argtypes = [vp, vp, ci, ci, ci, ci, vp, ci, ci, vp, vp, vp, ci]
    lines = []

    def measure(rec, call, counts):
        for _ in range(warm):
            call()
        times = []
        for _ in range(reps):
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record(stream)
            call()
            ev1.record(stream)
            ev1.synchronize()
            times.append(ev0.elapsed_time(ev1))
        rec.update(keypoints=counts(), reps=reps, ms_median=round(statistics.median(times), 4), ms_min=round(min(times), 4),
                   ms_max=round(max(times), 4), ms_median_per_image=round(statistics.median(times) / rec["images"], 4))
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    def fast(label, imgs, threshold, keep=None, cap=200000):
        nimg = len(imgs)
        h, w = imgs[0].shape[:2]
        c = 1 if imgs[0].ndim == 2 else imgs[0].shape[2]
        dev = [torch.from_numpy(im).cuda() for im in imgs]
        prm = capi.fast_params(threshold=threshold)
        out = torch.zeros(nimg * cap * 3, dtype=torch.float32, device="cuda")
        n = (C.c_int * nimg)()
        ptrs = (C.c_void_p * nimg)(*[d.data_ptr() for d in dev])
        xy, resp = C.c_void_p(out.data_ptr()), C.c_void_p(out.data_ptr() + 8 * nimg * cap)
        torch.cuda.synchronize()

        def call():
            if keep is None:
                rc = lib.svo_fast_detect_batch(ctx._h, ptrs, nimg, w, h, c, C.byref(prm), cap, xy, resp, None, n, capi.MEM_DEVICE)
            else:
                rc = lib.svo_fast_anms_batch(ctx._h, ptrs, nimg, w, h, c, C.byref(prm), keep, cap, xy, resp, n, capi.MEM_DEVICE)
            assert rc == 0, lib.svo_last_error()

        rec = {"fn": "svo_fast_detect_batch" if keep is None else "svo_fast_anms_batch", "case": label, "images": nimg,
               "size": f"{w}x{h}x{c}", "threshold": threshold, "keep": keep}
        measure(rec, call, lambda: list(n[:nimg]))

    def orb(label, imgs):
        dev = [torch.from_numpy(im).cuda() for im in imgs]
        h, w, c = imgs[0].shape
        got = []

        def call():
            got[:] = [ctx.orb_extract_batch_padded(dev)[0]]

        rec = {"fn": "svo_orb_extract_batch", "case": label, "images": len(imgs), "size": f"{w}x{h}x{c}",
               "note": "the whole extractor (8 levels, descriptors) through the Python wrapper"}
        measure(rec, call, lambda: [int(v) for v in got[0][:len(imgs)]])

    bgr = frames(16)
    grey = [np.ascontiguousarray(((f.astype(np.int64) * (1868, 9617, 4899)).sum(-1) + 8192 >> 14).astype(np.uint8)) for f in bgr]
    for t in (1, 20):
        fast(f"BGR, threshold {t}", bgr[:1], t)
        fast(f"BGR, threshold {t}, batch of 16", bgr, t)
        fast(f"grey, threshold {t}", grey[:1], t)
        fast(f"grey, threshold {t}, batch of 16", grey, t)
    for t in (1, 20):
        fast(f"BGR, threshold {t}, ANMS keep 4096", bgr[:1], t, keep=4096)
    fast("BGR, threshold 20, ANMS keep 4096, batch of 16", bgr, 20, keep=4096)
    orb("BGR", bgr[:1])
    orb("BGR, batch of 16", bgr)
    ctx.close()
    if args.out:
        pathlib.Path(args.out).write_text("".join(json.dumps(r) + "\n" for r in lines))


if __name__ == "__main__":
    main()
