"""svo_gftt_detect_batch alone on device inputs, with svo_fast_anms_batch on the same images beside it: HIP events recorded on the
context's stream around each call (which includes its waits for the counts), median of the repeats after warm-up.  1241 x 376 BGR,
batches of 1 and 16, min_distance 0 and 10, max_corners 1000 and quality 0.01 (GFTTDetector's defaults).  Prints JSON lines (--out:
also written there); each GFTT line carries the candidate counts and the rounds the selection needs per image (computed on the host
from the returned order by tests/gftt_numpy.py when --rounds is given: all pairs, slow).  Per-kernel times come from running this
script under a kernel trace in a run of its own (--brief: one repeat of each case, for that)."""
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--brief", action="store_true")
    ap.add_argument("--rounds", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    reps, warm = (1, 1) if args.brief else (args.reps, 5)
    torch.cuda.is_available()
    ctx = capi.Context(0)
    lib = ctx.lib
    stream = torch.cuda.ExternalStream(lib.svo_ctx_stream(ctx._h))
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

    def run(fn, label, imgs, prm, extra, cap=20000):
        nimg = len(imgs)
        h, w, c = imgs[0].shape
        dev = [torch.from_numpy(im).cuda() for im in imgs]
        out = torch.zeros(nimg * cap * 3, dtype=torch.float32, device="cuda")
        n = (C.c_int * nimg)()
        ptrs = (C.c_void_p * nimg)(*[d.data_ptr() for d in dev])
        xy, resp = C.c_void_p(out.data_ptr()), C.c_void_p(out.data_ptr() + 8 * nimg * cap)
        torch.cuda.synchronize()

        def call():
            if fn == "svo_gftt_detect_batch":
                rc = lib.svo_gftt_detect_batch(ctx._h, ptrs, None, nimg, w, h, c, C.byref(prm), cap, xy, resp, n, capi.MEM_DEVICE)
            else:
                rc = lib.svo_fast_anms_batch(ctx._h, ptrs, nimg, w, h, c, C.byref(prm), extra, cap, xy, resp, n, capi.MEM_DEVICE)
            assert rc == 0, lib.svo_last_error()

        rec = {"fn": fn, "case": label, "images": nimg, "size": f"{w}x{h}x{c}"}
        measure(rec, call, lambda: list(n[:nimg]))
        return rec

    bgr = frames(16)
    for md in (0.0, 10.0):
        for batch in (bgr[:1], bgr):
            prm = capi.gftt_params(min_distance=md)
            rec = run("svo_gftt_detect_batch", f"min_distance {md:g}, max_corners 1000", batch, prm, None)
            if args.rounds and md >= 1:
                import gftt_numpy as gn

                rec["candidates"], rec["rounds"] = [], []
                for im in batch[:2]:
                    idx, _, r = gn.candidates(gn.response(im), 0.01)
                    ys, xs = np.divmod(idx, im.shape[1])
                    rec["candidates"].append(r["n_candidates"])
                    rec["rounds"].append(gn.selection_rounds(xs, ys, md)[1] if len(idx) <= 12000 else None)
                print(json.dumps({"case": rec["case"], "images": rec["images"], "candidates": rec["candidates"], "rounds": rec["rounds"]}),
                      flush=True)
    for batch in (bgr[:1], bgr):
        run("svo_fast_anms_batch", "threshold 20, ANMS keep 1000", batch, capi.fast_params(threshold=20), 1000, cap=200000)
    ctx.close()
    if args.out:
        pathlib.Path(args.out).write_text("".join(json.dumps(r) + "\n" for r in lines))


if __name__ == "__main__":
    main()
