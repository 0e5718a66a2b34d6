"""svo_knn_match alone on device inputs: HIP events recorded on the context's stream around the call, warm-up calls first,
median of the repeats.  1000 x 1000 ORB descriptors (SVO_MATCH_L2_U8 on the 32 bytes, SVO_MATCH_HAMMING on the 8 words), 16 of
those as one batch, and 20000 x 20000 x 128 floats (SIFT::create(20000), src/StereoCV.cpp:65).  Prints JSON lines (--out: also
written there): achieved pair-elements per second -- an element is a float, a byte, or a 32-bit word of a binary descriptor
-- next to the VALU issue bound of the inner loop from the rates DESIGN.md section 6.3 measured (per wave64 instruction and
SIMD, two or more waves resident: v_fma_f32 1.0 ns, the integer dot class 1.75 ns; 1024 SIMDs).  The inner loops, from the
library's disassembly: float -- v_pk_add_f32 (the differences), v_pk_mul_f32, v_pk_add_f32 (two accumulators at a time): 1.5
instructions per element; bytes -- one v_dot4_u32_u8 per four elements; binary -- v_xor_b32 + v_bcnt_u32_b32 per word."""
import argparse
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
    ctx.close()
    if args.out:
        pathlib.Path(args.out).write_text("".join(json.dumps(r) + "\n" for r in lines))


if __name__ == "__main__":
    main()
