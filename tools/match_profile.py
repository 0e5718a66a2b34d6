"""svo_knn_match alone on device inputs: HIP events recorded on the context's stream around the call, warm-up calls first,
median of the repeats.  1000 x 1000 ORB descriptors (SVO_MATCH_L2_U8 on the 32 bytes, SVO_MATCH_HAMMING on the 8 words), 16 of
those as one batch, and 20000 x 20000 x 128 floats (SIFT::create(20000), src/StereoCV.cpp:65).  Prints JSON lines (--out: also
written there): achieved pair-elements per second -- an element is a float, a byte, or a 32-bit word of a binary descriptor
-- next to the VALU issue bound of the inner loop from the rates DESIGN.md section 6.3 measured (per wave64 instruction and
SIMD, two or more waves resident: v_fma_f32 1.0 ns, the integer dot class 1.75 ns; 1024 SIMDs).  The inner loops, from the
library's disassembly: float -- v_pk_add_f32 (the differences), v_pk_mul_f32, v_pk_add_f32 (two accumulators at a time): 1.5
instructions per element; bytes -- one v_dot4_u32_u8 per four elements; binary -- v_xor_b32 + v_bcnt_u32_b32 per word.

Then svo_match_cross, svo_knn_match_gated and svo_radius_match as whole calls on device inputs (wall clock, call + wait) beside what
svo_knn_match offers for the same job, at 1000 x 1000 ORB words, 2000 x 2000 SIFT floats and 10000 x 10000 BRIEF bytes: the
cross-check against two k = 1 searches, both lists copied to the host and paired in numpy; the gated search against the ungated
one; the radius search beside k = 4."""
import argparse
import ctypes
import json
import pathlib
import statistics
import sys

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from ros_stereo_slam_amd import capi  # noqa: E402

SIMDS, LANES = 1024, 64
# (instructions per pair-element, ns per wave64 instruction and SIMD)
BOUND = {capi.MATCH_L2_F32: (1.5, 1.0), capi.MATCH_L2_U8: (0.25, 1.75), capi.MATCH_HAMMING: (2.0, 1.0)}
NAMES = {capi.MATCH_L2_F32: "L2_F32", capi.MATCH_L2_U8: "L2_U8", capi.MATCH_HAMMING: "HAMMING"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():   # also loads the HIP runtime once, for torch and the library alike
        sys.exit("match_profile.py needs a GPU")
    ctx = capi.Context(0)
    lib = ctx.lib
    stream = torch.cuda.ExternalStream(lib.svo_ctx_stream(ctx._h))
    rng = np.random.default_rng(0)
    lines = []

    def timed(label, norm, nq, nt, dim, nprob, k=2):
        if norm == capi.MATCH_L2_F32:
            q, t = rng.normal(size=(nq * nprob, dim)).astype(np.float32), rng.normal(size=(nt * nprob, dim)).astype(np.float32)
        elif norm == capi.MATCH_L2_U8:
            q, t = rng.integers(0, 256, (nq * nprob, dim), np.uint8), rng.integers(0, 256, (nt * nprob, dim), np.uint8)
        else:
            q, t = (rng.integers(-2**31, 2**31, (n * nprob, dim), np.int64).astype(np.int32) for n in (nq, nt))
        dq, dt = torch.from_numpy(q).cuda(), torch.from_numpy(t).cuda()
        qo = np.ascontiguousarray(np.arange(nprob + 1) * nq, np.int32)
        to = np.ascontiguousarray(np.arange(nprob + 1) * nt, np.int32)
        idx = torch.empty((nq * nprob, k), dtype=torch.int32, device="cuda")
        dist = torch.empty((nq * nprob, k), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()

        def call():
            rc = lib.svo_knn_match(ctx._h, norm, capi._ptr(dq), capi._ptr(dt), dim, capi._ptr(qo), capi._ptr(to), nprob, k,
                                   capi._ptr(idx), capi._ptr(dist), capi.MEM_DEVICE)
            assert rc == 0, lib.svo_last_error()

        for _ in range(args.warmup):
            call()
        ctx.sync()
        times = []
        for _ in range(args.reps):
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record(stream)
            call()
            ev1.record(stream)
            ev1.synchronize()
            times.append(ev0.elapsed_time(ev1))
        ms = statistics.median(times)
        elements = float(nq) * nt * dim * nprob
        per_el, ns = BOUND[norm]
        bound = SIMDS * LANES / (per_el * ns * 1e-9)
        rec = {"fn": "svo_knn_match", "case": label, "norm": NAMES[norm], "problems": nprob, "queries": nq, "train": nt, "dim": dim,
               "k": k, "ms_median": round(ms, 4), "ms_min": round(min(times), 4), "ms_max": round(max(times), 4),
               "pair_elements_per_s": float(f"{elements / (ms * 1e-3):.4g}"), "valu_bound_pair_elements_per_s": float(f"{bound:.4g}"),
               "fraction_of_bound": round(elements / (ms * 1e-3) / bound, 4), "reps": args.reps, "warmup": args.warmup}
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    timed("ORB 1000 x 1000, bytes", capi.MATCH_L2_U8, 1000, 1000, 32, 1)
    timed("ORB 1000 x 1000, words", capi.MATCH_HAMMING, 1000, 1000, 8, 1)
    timed("batch 16 x (1000 x 1000), bytes", capi.MATCH_L2_U8, 1000, 1000, 32, 16)
    timed("batch 16 x (1000 x 1000), words", capi.MATCH_HAMMING, 1000, 1000, 8, 16)
    timed("SIFT 20000 x 20000 x 128", capi.MATCH_L2_F32, 20000, 20000, 128, 1)

    # ---- svo_match_cross, svo_knn_match_gated, svo_radius_match against what the parent's entry points offer ------------------
    # Wall-clock time of whole calls on device inputs (perf_counter around call + wait: the routes differ in what the host does),
    # the same warm-up and repeats; median, min and max per route.
    import time

    def wall(fn):
        for _ in range(args.warmup):
            fn()
        ctx.sync()
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            fn()
            ctx.sync()
            ts.append((time.perf_counter() - t0) * 1e3)
        return {"ms_median": round(statistics.median(ts), 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4)}

    def ext(label, norm, n, dim):
        if norm == capi.MATCH_L2_F32:
            q, t = rng.normal(size=(n, dim)).astype(np.float32), rng.normal(size=(n, dim)).astype(np.float32)
        elif norm == capi.MATCH_L2_U8:
            q, t = rng.integers(0, 256, (n, dim), np.uint8), rng.integers(0, 256, (n, dim), np.uint8)
        else:
            q, t = (rng.integers(-2**31, 2**31, (n, dim), np.int64).astype(np.int32) for _ in range(2))
        dq, dt = torch.from_numpy(q).cuda(), torch.from_numpy(t).cuda()
        xq = np.c_[rng.uniform(0, 1241, n), rng.uniform(0, 376, n)].astype(np.float32)
        xt = np.c_[rng.uniform(0, 1241, n), rng.uniform(0, 376, n)].astype(np.float32)
        dxq, dxt = torch.from_numpy(xq).cuda(), torch.from_numpy(xt).cuda()
        qo = np.array([0, n], np.int32)
        idx1, dist1 = (torch.empty(n, dtype=d, device="cuda") for d in (torch.int32, torch.float32))
        ridx, rdist = (torch.empty((n, 1), dtype=d, device="cuda") for d in (torch.int32, torch.float32))
        idx4, dist4 = (torch.empty((n, 4), dtype=d, device="cuda") for d in (torch.int32, torch.float32))
        p = capi._ptr
        head = (ctx._h, norm, p(dq), p(dt), dim, p(qo), p(qo), 1)
        swapped = (ctx._h, norm, p(dt), p(dq), dim, p(qo), p(qo), 1)

        def knn(args_, k, i, d):
            assert lib.svo_knn_match(*args_, k, p(i), p(d), capi.MEM_DEVICE) == 0, lib.svo_last_error()

        def cross(mode):
            assert lib.svo_match_cross(*head, mode, p(idx1), p(dist1), capi.MEM_DEVICE) == 0, lib.svo_last_error()

        def two_calls():    # the parent's route to a mutual cross-check: two searches, both lists to the host, numpy pairing
            knn(head, 1, ridx, rdist)
            ctx.sync()
            fwd = ridx.cpu().numpy()[:, 0]
            knn(swapped, 1, ridx, rdist)
            ctx.sync()
            back = ridx.cpu().numpy()[:, 0]
            return np.where(back[fwd] == np.arange(n), fwd, -1)

        gate = capi.MatchGate(2.0, 0.0, 128.0)

        def gated():
            assert lib.svo_knn_match_gated(*head, 2, None, p(dxq), p(dxt), ctypes.byref(gate), p(idx4), p(dist4), capi.MEM_DEVICE) == 0

        # a radius that keeps a handful of train rows per query: the fourth neighbour's median distance of the first 256 queries
        i10, d10 = ctx.knn_match(q[:256], t, k=4, norm=norm)
        radius = float(np.median(d10[:, 3]))
        cap = 64 * n
        cidx, cdist = (torch.empty(cap, dtype=d, device="cuda") for d in (torch.int32, torch.float32))
        coff = torch.empty(n + 1, dtype=torch.int32, device="cuda")
        total = ctypes.c_int()

        def radius_call():
            rc = lib.svo_radius_match(*head, ctypes.c_float(radius), p(coff), p(cidx), p(cdist), cap, ctypes.byref(total), capi.MEM_DEVICE)
            assert rc == 0, lib.svo_last_error()

        mutual = two_calls()
        cross(capi.CROSS_MUTUAL)
        ctx.sync()
        assert np.array_equal(idx1.cpu().numpy(), mutual), "svo_match_cross(MUTUAL) differs from the two-call route"
        for fn, call in (("svo_match_cross MUTUAL", lambda: cross(capi.CROSS_MUTUAL)), ("svo_match_cross CV", lambda: cross(capi.CROSS_CV)),
                         ("two svo_knn_match(k 1) + D2H + numpy pairing", two_calls),
                         ("svo_knn_match_gated k 2, band 2 rows x 128 columns", gated), ("svo_knn_match k 2", lambda: knn(head, 2, idx4, dist4)),
                         ("svo_radius_match", radius_call), ("svo_knn_match k 4", lambda: knn(head, 4, idx4, dist4))):
            rec = {"fn": fn, "case": label, "norm": NAMES[norm], "queries": n, "train": n, "dim": dim, **wall(call),
                   "reps": args.reps, "warmup": args.warmup}
            if fn == "svo_radius_match":
                rec.update(radius=round(radius, 4), matches=total.value)
            print(json.dumps(rec), flush=True)
            lines.append(rec)

    ext("ORB 1000 x 1000, words", capi.MATCH_HAMMING, 1000, 8)
    ext("SIFT 2000 x 2000 x 128", capi.MATCH_L2_F32, 2000, 128)
    ext("BRIEF 10000 x 10000, 32 bytes", capi.MATCH_L2_U8, 10000, 32)
    ctx.close()
    if args.out:
        pathlib.Path(args.out).write_text("".join(json.dumps(r) + "\n" for r in lines))


if __name__ == "__main__":
    main()
