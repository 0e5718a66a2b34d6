"""svo_sift_extract_batch alone on device inputs: HIP events recorded on the context's stream around the call (which includes its
one wait for the counts), median of the repeats.  1241 x 376 x 3 with n_features 10000 and 20000, 640 x 240 x 3, a 2-image batch
at 1241 x 376, detection without descriptors, and svo_sift_pyramid's share (the scale space alone).  Prints JSON lines (--out:
also written there)."""
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

SIZES = {"640x240": ((640, 240), (360.0, 360.0, 320.0, 120.0)), "1241x376": ((1241, 376), (718.856, 718.856, 607.1928, 185.2157))}


def frame(size_key, k=0):
    size, K4 = SIZES[size_key]
    R, t = synth.corridor_trajectory(k + 1, step=0.5)[k]
    return np.ascontiguousarray(synth.Scene().render(R, t, K=K4, size=size, channels=3)[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.is_available()
    ctx = capi.Context(0)
    lib = ctx.lib
    stream = torch.cuda.ExternalStream(lib.svo_ctx_stream(ctx._h))
    # every pointer goes in as a pointer: without argtypes ctypes passes a plain Python int as a 32-bit C int
    vp, ci = C.c_void_p, C.c_int
    lib.svo_sift_pyramid.argtypes = [vp, vp, ci, ci, ci, vp, vp, vp, ci]
    lib.svo_sift_extract_batch.argtypes = [vp, vp, ci, ci, ci, ci, vp, ci, vp, vp, vp, vp, vp, vp, vp, ci]
    lines = []

    def timed(label, frames, n_features, cap=40000, descriptors=True, pyramid_only=False):
        imgs = [torch.from_numpy(f).cuda() for f in frames]
        nimg = len(imgs)
        h, w, c = frames[0].shape
        prm = capi.sift_params(n_features=n_features)
        e = nimg * cap
        fb = torch.zeros(e * 133, dtype=torch.float32, device="cuda")
        ob = torch.zeros(e, dtype=torch.int32, device="cuda")
        n = (C.c_int * nimg)()
        ptrs = (C.c_void_p * nimg)(*[im.data_ptr() for im in imgs])
        base = fb.data_ptr()
        if pyramid_only:
            no, ow, oh = C.c_int(), (C.c_int * 16)(), (C.c_int * 16)()
            assert lib.svo_sift_pyramid_layout(w, h, 3, C.byref(no), ow, oh) == 0
            px = sum(ow[o] * oh[o] for o in range(no.value))
            gd = torch.zeros(px * 11, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()

        def call():
            if pyramid_only:
                rc = lib.svo_sift_pyramid(ctx._h, C.c_void_p(imgs[0].data_ptr()), w, h, c, C.byref(prm), C.c_void_p(gd.data_ptr()),
                                          C.c_void_p(gd.data_ptr() + 4 * px * 6), capi.MEM_DEVICE)
            else:
                rc = lib.svo_sift_extract_batch(ctx._h, ptrs, nimg, w, h, c, C.byref(prm), cap, C.c_void_p(base),
                                                C.c_void_p(base + 8 * e), C.c_void_p(base + 12 * e), C.c_void_p(base + 16 * e),
                                                capi._ptr(ob), C.c_void_p(base + 20 * e if descriptors else 0), n, capi.MEM_DEVICE)
            assert rc == 0, lib.svo_last_error()

        for _ in range(3):
            call()
        times = []
        for _ in range(args.reps):
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record(stream)
            call()
            ev1.record(stream)
            ev1.synchronize()
            times.append(ev0.elapsed_time(ev1))
        rec = {"fn": "svo_sift_pyramid" if pyramid_only else "svo_sift_extract_batch", "case": label, "images": nimg,
               "size": f"{w}x{h}x{c}", "n_features": n_features, "descriptors": bool(descriptors and not pyramid_only),
               "keypoints": [] if pyramid_only else list(n[:nimg]), "ms_median": round(statistics.median(times), 4),
               "ms_min": round(min(times), 4), "ms_max": round(max(times), 4)}
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    big, small = frame("1241x376"), frame("640x240")
    timed("1241x376 n_features 10000", [big], 10000)
    timed("1241x376 n_features 20000", [big], 20000)
    timed("640x240 n_features 10000", [small], 10000)
    timed("2 x 1241x376 n_features 10000", [big, frame("1241x376", 1)], 10000)
    timed("1241x376 detect only", [big], 10000, descriptors=False)
    timed("1241x376 scale space only (copies of the layers included)", [big], 0, pyramid_only=True)
    ctx.close()
    if args.out:
        pathlib.Path(args.out).write_text("".join(json.dumps(r) + "\n" for r in lines))


if __name__ == "__main__":
    main()
