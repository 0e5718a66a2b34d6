#!/usr/bin/env python3
"""Time of svo_replenish beside the six-call composition it replaces (svo_dedup_points -> svo_compact -> svo_transform_points ->
a host z > 0 mask -> svo_compact -> concatenation), on device-resident sets, at the prototype's size (2 000 new points against
8 192 held) and at the library's caps (20 000 against 65 536), both modes.

Every figure is a host clock around calls that end in a wait for the device (the composition waits three times by itself: it needs
the survivor count and the z column on the host), the median of --repeat alternating rounds after --warmup rounds; the two results
are compared bit for bit before anything is timed.  Needs an MI355X; there is no CPU path.  One JSON line per case goes to stdout
and, with --out, to a file."""
import argparse
import ctypes as C
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def make_case(n_ref, n_new, seed):
    """Pixels of a 1241 x 376 image (quarter-pixel lattice), depths on both sides of the camera."""
    rng = np.random.default_rng(seed)
    ref = np.stack([rng.integers(4, 1241 * 4, n_ref) / 4.0, rng.integers(4, 376 * 4, n_ref) / 4.0], axis=1).astype(np.float32)
    new = np.stack([rng.integers(4, 1241 * 4, n_new) / 4.0, rng.integers(4, 376 * 4, n_new) / 4.0], axis=1).astype(np.float32)
    ref3 = rng.normal(0, 5, (n_ref, 3)).astype(np.float32)
    new3 = np.stack([rng.normal(0, 5, n_new), rng.normal(0, 2, n_new), rng.uniform(-2, 40, n_new)], axis=1).astype(np.float32)
    a = 0.05
    Rt = np.array([[np.cos(a), 0, np.sin(a), 0.3], [0, 1, 0, -0.1], [-np.sin(a), 0, np.cos(a), -1.0]])
    return ref, ref3, new, new3, np.ascontiguousarray(Rt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--radius", type=float, default=5.0)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("replenish_profile: no GPU; a time measured anywhere else would say nothing")
    from ros_stereo_slam_amd import capi

    ctx = capi.Context(0)
    lib, h, p = ctx.lib, ctx._h, capi._ptr
    lines = []
    for n_ref, n_new in ((8192, 2000), (65536, 20000)):
        for mode, mode_name in ((capi.DEDUP_BOX, "box"), (capi.DEDUP_DISC, "disc")):
            ref, ref3, new, new3, Rt = make_case(n_ref, n_new, 1)
            cap = n_ref + n_new
            dev = lambda a: torch.from_numpy(a).cuda()
            d_new, d_new3 = dev(new), dev(new3)
            hold = lambda a, w: torch.cat([dev(a), torch.zeros((n_new, w), dtype=torch.float32, device="cuda")])
            one_xy, one_xyz, six_xy, six_xyz = hold(ref, 2), hold(ref3, 3), hold(ref, 2), hold(ref3, 3)
            counts = torch.zeros(3, dtype=torch.int32, device="cuda")
            keep = torch.zeros(n_new, dtype=torch.uint8, device="cuda")
            k_cnt = torch.zeros(2, dtype=torch.int32, device="cuda")
            t_xy, t_xyz, t_moved = (torch.zeros((n_new, w), dtype=torch.float32, device="cuda") for w in (2, 3, 3))
            torch.cuda.synchronize()

            def one_call():
                capi._check(lib.svo_replenish(h, p(one_xy), p(one_xyz), n_ref, cap, p(d_new), p(d_new3), n_new, C.c_double(args.radius),
                                              mode, p(Rt), C.c_void_p(counts.data_ptr()), C.c_void_p(counts.data_ptr() + 4),
                                              C.c_void_p(counts.data_ptr() + 8), capi.MEM_DEVICE))
                ctx.sync()
                return int(counts[0].item())

            def six_calls():
                capi._check(lib.svo_dedup_points(h, p(six_xy), n_ref, None, 0, p(d_new), n_new, C.c_double(args.radius), mode, p(keep),
                                                 None, capi.MEM_DEVICE))
                capi._check(lib.svo_compact(h, p(keep), n_new, p(d_new), 2, p(t_xy), p(d_new3), 3, p(t_xyz), None, 0, None,
                                            C.c_void_p(k_cnt.data_ptr()), capi.MEM_DEVICE))
                ctx.sync()
                k = int(k_cnt[0].item())                                       # the host has to know how many to move
                capi._check(lib.svo_transform_points(h, p(Rt), p(t_xyz), k, p(t_moved), capi.MEM_DEVICE))
                ctx.sync()
                front = (t_moved[:k, 2].cpu().numpy() > 0).astype(np.uint8)   # the host z > 0 mask
                d_front = torch.from_numpy(front).cuda() if k else keep
                torch.cuda.synchronize()
                capi._check(lib.svo_compact(h, p(d_front), k, p(t_xy), 2, C.c_void_p(six_xy.data_ptr() + 8 * n_ref), p(t_moved), 3,
                                            C.c_void_p(six_xyz.data_ptr() + 12 * n_ref), None, 0, None,
                                            C.c_void_p(k_cnt.data_ptr() + 4), capi.MEM_DEVICE))      # written in place: the concatenation
                ctx.sync()
                return n_ref + (int(k_cnt[1].item()) if k else 0)

            def dedup_only():
                capi._check(lib.svo_dedup_points(h, p(one_xy), n_ref, None, 0, p(d_new), n_new, C.c_double(args.radius), mode, p(keep),
                                                 None, capi.MEM_DEVICE))
                ctx.sync()

            n_one, n_six = one_call(), six_calls()
            same = n_one == n_six and torch.equal(one_xy[:n_one], six_xy[:n_six]) and torch.equal(one_xyz[:n_one], six_xyz[:n_six])
            if not same:
                raise SystemExit(f"replenish_profile: the two results differ at {n_ref} / {n_new} {mode_name}")
            times = {"replenish": [], "composition": [], "dedup_only": []}
            for r in range(args.warmup + args.repeat):
                for name, fn in (("replenish", one_call), ("composition", six_calls), ("dedup_only", dedup_only)):
                    t0 = time.perf_counter()
                    fn()
                    dt = time.perf_counter() - t0
                    if r >= args.warmup:
                        times[name].append(dt * 1e3)
            rec = {"n_ref": n_ref, "n_new": n_new, "mode": mode_name, "radius": args.radius, "n_out": n_one,
                   "n_dup": int(counts[1].item()), "n_behind": int(counts[2].item()), "repeat": args.repeat, "warmup": args.warmup,
                   "bit_identical": bool(same), "device": torch.cuda.get_device_name(0)}
            for name, v in times.items():
                v = np.array(v)
                rec[name + "_ms_median"] = round(float(np.median(v)), 4)
                rec[name + "_ms_p10"] = round(float(np.percentile(v, 10)), 4)
                rec[name + "_ms_p90"] = round(float(np.percentile(v, 90)), 4)
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
