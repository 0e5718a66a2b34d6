#!/usr/bin/env python3
"""A robust optimise against a plain one on the same graph: tools/pg_profile.py's V vertices on the benchmark loop with drift and C
identity closures, 10 Gauss-Newton iterations, device-timed (HIP events inside the library, SVO_K_POSEGRAPH), medians over
`repeats` fresh graphs after one warm-up.  "plain": no kernel stored, the non-robust linearisation; "robust": Geman-McClure on
every closure (svo_pg_set_loop_closure_kernel), the robust linearisation; "unit": the same with a parameter so large that every
weight is 1.0 -- the plain solve's arithmetic through the robust kernel.  One JSON line per variant.
    python tools/pg_robust_profile.py [V] [C] [repeats] [mu]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

torch.cuda.is_available()
from ros_stereo_slam_amd import capi, chunked, synth

V = int(sys.argv[1]) if len(sys.argv) > 1 else 4541
Cn = int(sys.argv[2]) if len(sys.argv) > 2 else 40
rep = int(sys.argv[3]) if len(sys.argv) > 3 else 9
mu = float(sys.argv[4]) if len(sys.argv) > 4 else 1.0
ITERS = 10
poses = synth.loop_trajectory(V, **synth.BENCH_LOOP)
R0, t0 = poses[0]
rng = np.random.default_rng(1)
traj, drift = [], np.zeros(3)
for R, t in poses:
    drift = drift + rng.normal(0, 0.002, 3)
    traj.append((R0.T @ R, R0.T @ (t - t0) + drift))
matches = synth.loop_closures(poses, max_dist=0.3, max_angle_deg=10.0, min_gap=100, pick="nearest")
closures = chunked.gate_closures([m if m >= 1 else -1 for m in matches])
closures = dict(list(closures.items())[:Cn])
ctx = capi.Context(0)
ctx.enable_kernel_timing(True)
VARIANTS = {"plain": None, "robust": (capi.PG_ROBUST_GEMAN_MCCLURE, mu), "unit": (capi.PG_ROBUST_GEMAN_MCCLURE, 1e30)}
ref = None
for name, kernel in VARIANTS.items():
    ms, chi = [], None
    for r in range(rep + 1):
        pg = capi.PoseGraph(ctx)
        if kernel:
            pg.set_loop_closure_kernel(*kernel)
        ctx.reset_kernel_time()
        est, chi = chunked.global_solve(pg, traj, closures, iters=ITERS)
        if r:                                   # the first graph pays for code loading and allocation
            ms.append(ctx.kernel_time(capi.K_POSEGRAPH)[0] / ITERS)
        w = pg.edge_residuals()[1] if kernel else np.ones(pg.num_edges)
        pg.close()
    if name == "plain":
        ref = est
    ms = np.array(ms)
    print(json.dumps(dict(variant=name, vertices=V, closures=len(closures), iterations=ITERS, repeats=rep,
                          ms_per_iteration_median=round(float(np.median(ms)), 4), ms_min=round(float(ms.min()), 4),
                          ms_max=round(float(ms.max()), 4), chi2_first=float(chi[0]), chi2_last=float(chi[-1]),
                          weights_below_1=int((w < 1).sum()), min_weight=float(w.min()),
                          same_bits_as_plain=bool(np.array_equal(est, ref)))), flush=True)
ctx.close()
