#!/usr/bin/env python3
"""Timing of the ICP entry points (csrc/cloud.hip): one pairwise registration of two 4096-point keyframe clouds and of two
2^18-point dense clouds, per stage -- index build, normals (kNN + eigenvectors), one search of every source point, one
step's normal equations, the information matrix, and the whole pairwise call with its iteration counts.  Wall time around
synchronising calls, after one untimed warm-up, median of --repeat runs.  One JSON line per size.
    python tools/icp_profile.py [--repeat 5] [--out profiles/icp_profile.jsonl]"""
import argparse
import json
import pathlib
import sys
import time

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))


def surface(n, seed):
    """n points on three perpendicular, noisy planes (a corridor corner), metres"""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 3, n)
    uv = 10 + 6 * rng.random((n, 2))
    p = np.full((n, 3), 10.0) + rng.normal(0, 0.005, (n, 3))
    for a in range(3):
        m = k == a
        p[np.ix_(m, [b for b in range(3) if b != a])] = uv[m]
    return p


def med(fn, repeat):
    fn()
    ts = []
    for _ in range(repeat):
        t = time.perf_counter()
        r = fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts)), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch

    torch.cuda.is_available()
    from ros_stereo_slam_amd import capi

    ctx = capi.Context(0)
    c, s = np.cos(0.01), np.sin(0.01)
    Ti = np.array([[c, -s, 0, 0.05], [s, c, 0, -0.03], [0, 0, 1, 0.04]])
    lines = []
    for n in (4096, 1 << 18):
        tgt = surface(n, 1).astype(np.float32)
        q = surface(n, 2)
        src = (q @ Ti[:, :3].T + Ti[:, 3]).astype(np.float32)
        rec = dict(n=n, repeat=a.repeat)
        rec["cloud_create_ms"], cloud = med(lambda: capi.Cloud(ctx, tgt), a.repeat)

        def nrm():
            cloud.estimate_normals(30)
            ctx.sync()

        rec["normals_knn30_ms"], _ = med(nrm, a.repeat)
        rec["search_all_sources_ms"], _ = med(lambda: ctx.icp_correspondences(src, cloud, 1.5), a.repeat)
        rec["one_step_ms"], _ = med(lambda: ctx.icp_normal_equations(src, cloud, 1.5), a.repeat)
        rec["information_ms"], _ = med(lambda: ctx.icp_information(src, cloud, 1.5), a.repeat)
        rec["pairwise_ms"], (T, L, d) = med(lambda: ctx.icp_pairwise(src, cloud, 15.0, 1.5), a.repeat)
        rec["iterations"] = [int(v) for v in d["iterations"]]
        rec["fitness"] = [float(v) for v in d["fitness"]]
        rec["rmse"] = [float(v) for v in d["rmse"]]
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        cloud.close()
    if a.out:
        pathlib.Path(a.out).write_text("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
