#!/usr/bin/env python3
"""bench.py -- stereo frames/s of the MI355X front-end on a synthetic 1241x376 stream.

Contract (driver): ``python bench.py --gpus N --steps K --warmup W`` prints ONE JSON line on
rank 0.  A step is one pass of the hot path over one batch of stereo frames whose images are
already resident in HBM: one frame of every chunk this GPU keeps in flight, each through the
pyramid of the new left image, pyramidal LK of the reference keypoints, F-matrix RANSAC,
PnP-RANSAC + refinement, pose composition, keyframe rule and -- when the rule fires -- the stereo
keyframe path (right pyramid, grid + ANMS to 4096 keypoints, LK left->right, F-RANSAC, DLT
triangulation, rigid transform).  That is BASELINE.json configs[1] ("front-end only, pose-graph
off") on the synthetic stream of SURVEY.md 8d.

The stream is ONE walk of the generator's rounded-rectangle loop (0.9 m per frame, a lap of 492
frames), cut into contiguous chunks with one frame of overlap: rank r owns frames
[r*M*L, (r+1)*M*L], chunk m of it frames [m*L, (m+1)*L] with L = warmup + steps; every chunk
re-initialises at its first frame.  The warm-up steps are the first W frames of every chunk, the K
timed steps the next K.  The one exchange step of the path -- the all-gather of the chunk-boundary
poses, 12 doubles per chunk, RCCL for N > 1 -- is inside the timed region.  Weak scaling.

A plain run does only what the headline needs: set-up, the W warm-up steps, the K timed steps ONCE
(``ms_per_step`` = the clock over them / K), the outputs (``--dump-outputs DIR``) and the line.
``--full`` adds everything below: the timed region repeated until ``--min-timed-s`` is on the clock,
the instrumented pass behind ``roofline`` and the stage table, the legs beyond the front-end's clock
and the CPU baseline.

``--dump-outputs DIR`` writes, after the timed steps, what the timed path returned to its caller at
its last step (rank 0's chunks) and the chunk start poses of the exchange, as float64 ``.npy`` files:
last_step_{R,t,inliers,tracked,keyframe} and chunk_start_{R,t}.  The inputs are the same on every run
with the same arguments (seeded generator, no clock in them).

Reported beside ``value`` with ``--full`` (all measured in this invocation, nothing carried as a literal):
  value_including_chunk_inits  the whole share again, every chunk's stereo initialisation included
  single_chunk_frames_per_s    ONE contiguous chunk per GPU (the north-star's partitioning),
                               pipelined, over rank 0's whole share
  ate_*                        trajectory error of the stitched 64*N-chunk run and of the
                               sequential run against the generator's truth, against each other,
                               and of the GPU against the CPU oracle on the frames the oracle ran
  posegraph_ms_per_iter        configs[3]'s global solve on the stitched trajectory with the
                               generator's loop closures (one svo_pg_optimize, 10 GN iterations)
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

# One hardware queue per context stream plus room for the default stream (torch's copies) and for
# the streams RCCL creates in a multi-GPU run.  Must be set before the HIP
# runtime initialises, i.e. before torch is imported.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

W, H, C = 1241, 376, 3
PYR_BYTES = 619930 * C    # sum of the 4 level sizes
LK_PMC_JSON = os.path.join(ROOT, "profiles", "r05_lk_pmc_{kpts}.json")   # one per keypoint count (4096, 8192)


def lk_algorithmic_bytes(n_pts: int) -> int:
    """HBM bytes one LK pass must move: both pyramids once + 8 B in / 13 B out per point
    (the LK share of SURVEY 8d's B_track = 3*pyr + 71*N)."""
    return 2 * PYR_BYTES + 21 * n_pts


def frame_algorithmic_bytes(n_pts: int, keyframe_rate: float) -> float:
    return 3 * PYR_BYTES + 71 * n_pts + keyframe_rate * (3 * PYR_BYTES + 102 * n_pts)


def lk_pmc_constants(n_kpts: int):
    """Per-pass counter figures of lk_track_kernel<3> from the committed rocprofv3 --pmc passes
    (tools/pmc_summary.py --json writes the file next to the CSVs).  They are only valid for the
    build and workload they were taken on: the file names the sha256 of lk.hip and the keypoint
    count, anything else gives None."""
    try:
        with open(LK_PMC_JSON.format(kpts=n_kpts)) as f:
            d = json.load(f)
        with open(os.path.join(ROOT, "ros_stereo_slam_amd", "csrc", "lk.hip"), "rb") as f:
            sha = hashlib.sha256(f.read()).hexdigest()
    except (OSError, ValueError):
        return None
    if d.get("lk_hip_sha256") != sha or d.get("kpts") != n_kpts:
        return None
    return d


def render_stream(scene, poses, device: str, batch: int = 8):
    """``synth.stereo_torch(scene, poses, device=device, batch=batch)`` with every distinct pose ray-cast once.  The bench
    loop is closed (a lap of 492 frames): past the first lap each pose repeats an earlier one bit for bit, and the renderer
    is a per-pixel function of the pose, so a repeat's images are copies of the first render.  The stream is laid out as
    stereo_torch lays it out (one tensor per batch of frames: its left images, then its right images)."""
    import torch
    from ros_stereo_slam_amd import synth

    keys = [np.asarray(R, np.float64).tobytes() + np.asarray(t, np.float64).tobytes() for R, t in poses]
    slot, uniq = {}, []
    for p, k in zip(poses, keys):
        if k not in slot:
            slot[k] = len(uniq)
            uniq.append(p)
    ul, ur = synth.stereo_torch(scene, uniq, device=device, batch=batch)
    lefts, rights = [], []
    for s in range(0, len(poses), batch):
        js = [slot[k] for k in keys[s:s + batch]]
        if js == list(range(s, s + len(js))):     # first renders: stereo_torch's own batch
            lefts.extend(ul[j] for j in js)
            rights.extend(ur[j] for j in js)
            continue
        both = torch.stack([ul[j] for j in js] + [ur[j] for j in js])
        lefts.extend(both[i] for i in range(len(js)))
        rights.extend(both[len(js) + i] for i in range(len(js)))
    return lefts, rights


def rel_truth(poses):
    """Generator poses relative to the first one (the VO's frame): [(R, t)]."""
    R0, t0 = poses[0]
    return [(R0.T @ R, R0.T @ (t - t0)) for R, t in poses]


def rot_angle(Ra, Rb):
    return float(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1) / 2, -1, 1)))


def kitti_leg(args):
    """BASELINE configs[0-3] take a KITTI odometry directory from the CLI; the data
    is not in the reference checkout nor on the GPU box, so this leg normally reports its absence."""
    from ros_stereo_slam_amd import sequence

    seq_dir = os.path.join(args.kitti, "sequences", args.seq)
    if not os.path.isdir(seq_dir):
        print(json.dumps({"skipped": "KITTI data absent", "looked_in": seq_dir,
                          "config": {"workload": f"KITTI odometry sequence {args.seq} (BASELINE configs[0-3])"}}))
        return 0
    return sequence.bench_kitti(args, seq_dir)


def free_port() -> int:
    import socket

    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def launch_ranks(n: int) -> int:
    """``python bench.py --gpus N`` without a launcher: start N fresh rank processes -- one per GPU,
    RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* in their environment, exactly what
    ``python -m torch.distributed.run --nproc-per-node N`` would give them -- wait for all of them, forward
    rank 0's single JSON line and fail if any rank failed.  This process never initialises the GPU
    (no torch import, no HIP call): the ranks are children, not a replacement of this process."""
    import subprocess

    port = os.environ.get("MASTER_PORT") or str(free_port())
    procs = []
    for r in range(n):
        env = dict(os.environ)
        env.update({"RANK": str(r), "LOCAL_RANK": str(r), "WORLD_SIZE": str(n), "LOCAL_WORLD_SIZE": str(n),
                    "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": port, "HSA_ENABLE_IPC_MODE_LEGACY": "0"})
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL, text=True))
    # rank 0's stdout is drained by a thread, so that every rank can be polled: a rank that dies before the rendezvous
    # must not leave the others (and this launcher) waiting for torch's store timeout
    import threading

    chunks0 = []
    reader = threading.Thread(target=lambda: chunks0.append(procs[0].stdout.read()), daemon=True)
    reader.start()
    codes = [None] * n
    failed = None
    while any(c is None for c in codes):
        for r, q in enumerate(procs):
            if codes[r] is None:
                codes[r] = q.poll()
                if codes[r] not in (None, 0) and failed is None:
                    failed = r
        if failed is not None:
            for r, q in enumerate(procs):
                if codes[r] is None:
                    q.terminate()
            for r, q in enumerate(procs):
                if codes[r] is None:
                    try:
                        codes[r] = q.wait(timeout=20)
                    except subprocess.TimeoutExpired:
                        q.kill()
                        codes[r] = q.wait()
            break
        time.sleep(0.05)
    reader.join(timeout=10)
    out0 = "".join(c for c in chunks0 if c)
    if failed is not None:
        print(f"bench.py: rank {failed} exited with code {codes[failed]}; the other ranks were stopped", file=sys.stderr)
    lines = [ln for ln in (out0 or "").splitlines() if ln.strip()]
    json_lines = [ln for ln in lines if ln.lstrip().startswith("{")]
    for ln in lines:
        if ln not in json_lines:
            print(ln, file=sys.stderr)      # anything else rank 0 wrote is not the contract's line
    if any(codes):
        print(f"bench.py: rank exit codes {codes}", file=sys.stderr)
        return (codes[failed] if failed is not None else next(c for c in codes if c)) or 1
    if len(json_lines) != 1:
        print(f"bench.py: rank 0 printed {len(json_lines)} JSON lines, expected one", file=sys.stderr)
        return 1
    print(json_lines[0])
    return 0


def launcher_selftest(rank: int, world: int) -> int:
    """SVO_BENCH_LAUNCHER_SELFTEST=1 (tests/test_bench_launcher.py, runs without a GPU): the rank only joins
    the rendezvous over gloo, takes part in one real all-gather and rank 0 prints the line's launcher-relevant
    keys -- the proof that ``--gpus N`` starts N ranks."""
    import torch
    import torch.distributed as dist

    if world > 1:
        dist.init_process_group("gloo")
        got = [torch.zeros(1, dtype=torch.int64) for _ in range(world)]
        dist.all_gather(got, torch.tensor([rank], dtype=torch.int64))
        seen = sorted(int(g.item()) for g in got)
        assert seen == list(range(world)), seen
        ranks_seen = dist.get_world_size()
        dist.barrier()
        dist.destroy_process_group()
    else:
        ranks_seen = 1
    if os.environ.get("SVO_BENCH_SELFTEST_FAIL_RANK") == str(rank):
        return 3
    if rank == 0:
        print(json.dumps({"metric": "launcher selftest", "n_gpus": world, "ranks_seen": ranks_seen}))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50,
                    help="timed steps; one step = one frame of every chunk of the GPU (64 frames per GPU with the defaults)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline: repeats up to --min-timed-s, the instrumented pass (roofline, stage "
                         "table), the legs beyond the front-end's clock and the CPU baseline; the --no-* options below trim it")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the timed path returned at its last step as DIR/<name>.npy (float64)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-extras", action="store_true",
                    help="only the contract's timed region (no re-run with inits, no single-chunk run, no pose graph)")
    ap.add_argument("--pipeline", choices=("auto", "on", "off"), default="auto",
                    help="two-stream overlap of PnP(t) with pyramid + LK(t+1) inside a chunk; auto = on for one "
                         "chunk per GPU, off when several chunks already fill the hardware queues")
    ap.add_argument("--chunks-per-gpu", type=int, default=int(os.environ.get("SVO_CHUNKS_PER_GPU", "64")),
                    help="contiguous chunks of this GPU's share of the stream run side by side (svo_vo_run_chunks)")
    ap.add_argument("--chunks-per-context", type=int, default=int(os.environ.get("SVO_CHUNKS_PER_CONTEXT", "16")),
                    help="chunks that share one context (= one stream): advanced in lock step, every stage of the "
                         "tracking path ONE set of launches for all of them (1..16)")
    ap.add_argument("--kpts", type=int, default=4096, choices=(4096, 8192),
                    help="keypoints per frame: 4096 = BASELINE's metric (grid step 10), 8192 = configs[4] shape "
                         "(grid step 7 -> 9152 lattice points -> ANMS 8192, keyframe rule 4000)")
    ap.add_argument("--no-kpts8192", action="store_true", help="skip the 8192-keypoint leg of the default run")
    ap.add_argument("--no-host-images", action="store_true", help="skip the leg that takes the frames from pinned host memory")
    ap.add_argument("--cpu-frames", type=int, default=24)
    ap.add_argument("--no-detector", action="store_true",
                    help="pose-graph leg: take the loop closures from the generator instead of running the detector")
    ap.add_argument("--no-kernel-timing", action="store_true",
                    help="diagnostic: no HIP events around the kernels (the roofline object is then empty)")
    ap.add_argument("--min-timed-s", type=float, default=1.0,
                    help="--full: the K timed steps are repeated (warm-up untimed every time) until this much time is on the clock")
    ap.add_argument("--max-repeats", type=int, default=16)
    ap.add_argument("--kitti", default=None, help="KITTI odometry root (holds sequences/<seq>/image_2, image_3)")
    ap.add_argument("--seq", default="00")
    args = ap.parse_args()
    if not args.full:
        # the headline alone: the K timed steps once, nothing measured beside them.  An option that only shapes what
        # --full adds is refused rather than silently dropped.
        full_only = [f"--{d.replace('_', '-')}" for d in ("no_cpu_baseline", "no_extras", "no_kpts8192", "no_host_images",
                                                          "cpu_frames", "no_detector", "no_kernel_timing", "min_timed_s",
                                                          "max_repeats")
                     if getattr(args, d) != ap.get_default(d)]
        if full_only:
            ap.error(f"{', '.join(full_only)} only apply with --full")
        args.no_extras = args.no_kernel_timing = args.no_cpu_baseline = True
        args.min_timed_s = 0.0
    if args.kitti is not None:
        return kitti_leg(args)
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        return launch_ranks(args.gpus)      # the ranks are children; this process stays off the GPU
    if os.environ.get("SVO_BENCH_LAUNCHER_SELFTEST") == "1":
        return launcher_selftest(int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1")))

    import torch

    n_kpts, grid_step, kf_min = (4096, 10, 2000) if args.kpts == 4096 else (8192, 7, 4000)

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    t_start = time.perf_counter()

    def trace(what: str):
        """SVO_BENCH_TRACE=1: one stderr line per leg and rank (where a run is when it is slow, or where it stopped)"""
        if os.environ.get("SVO_BENCH_TRACE") == "1":
            print(f"[bench rank {rank} +{time.perf_counter() - t_start:7.1f} s] {what}", file=sys.stderr, flush=True)

    # Rehearsal of the N > 1 path on a ONE-GPU box (never used by the driver): all ranks share
    # device 0 and the collectives run over gloo on host tensors.
    rehearsal = os.environ.get("SVO_BENCH_REHEARSE_ON_ONE_GPU") == "1"
    if rehearsal:
        local_rank = 0
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the HIP path has no CPU fallback")
    torch.cuda.set_device(local_rank)
    # Control traffic (barriers, max over ranks, the trajectory gather) runs over gloo on host tensors; the path's ONE
    # data collective -- the all-gather of chunk-boundary poses -- runs over RCCL through the C ABI (a communicator the
    # library makes, below).  No RCCL communicator exists in the process before the single-chunk leg has run: a live one
    # holds hardware queues and costs that leg a quarter of its rate.
    dist = None
    if world > 1:
        import torch.distributed as dist_mod

        dist = dist_mod
        dist.init_process_group("gloo")
    coll_dev = "cpu"
    from ros_stereo_slam_amd import capi, chunked, synth

    M = max(1, args.chunks_per_gpu)
    G = max(1, min(16, args.chunks_per_context))
    Wn, K = max(0, args.warmup), max(1, args.steps)
    L = Wn + K                       # frame-to-frame transitions per chunk
    share = M * L                    # transitions per rank
    pipeline = args.pipeline == "on" or (args.pipeline == "auto" and M == 1)
    scene = synth.bench_scene()
    poses_all = synth.loop_trajectory(world * share + 1, **synth.BENCH_LOOP)
    my_poses = poses_all[rank * share:(rank + 1) * share + 1]
    t_r0 = time.perf_counter()
    lefts, rights = render_stream(scene, my_poses, device=f"cuda:{local_rank}", batch=8)
    torch.cuda.synchronize()
    render_s = time.perf_counter() - t_r0

    vo_kw = dict(grid_step=grid_step, anms_keep=n_kpts, keyframe_min_inliers=kf_min)
    sh = chunked.ShardedVO(capi, local_rank, W, H, C, M, G, first_chunk_id=rank * M, seed=20261003, **vo_kw)
    bounds = chunked.chunk_bounds(share + 1, M)
    assert all(e - s == L for s, e in bounds)

    comm_state = {"thread": None}

    def make_communicator():
        """The path's one collective behind the C ABI: an RCCL communicator made by the library itself (what a C++ host
        of INTEGRATION.md section 6 uses), on a context of its OWN; the 128-byte id travels over gloo.  If any rank
        cannot make it, all ranks agree on the next form: a torch.distributed nccl (= RCCL) group, then gloo.
        -> (comm or None, torch group or None, text for config.collective)"""
        if world == 1:
            return None, None, ("none: one rank (tests/test_gpu_sharded.py runs svo_shard_allgather_boundaries on a "
                                "one-rank communicator)")
        if rehearsal and os.environ.get("SVO_BENCH_REHEARSE_CABI") != "1":
            return None, None, "gloo rehearsal on one GPU"
        comm, why = None, ""
        if os.environ.get("SVO_BENCH_NO_CABI") == "1":
            why = "SVO_BENCH_NO_CABI=1"
        else:
            ident = None
            if rank == 0:
                try:
                    ident = capi.shard_unique_id()
                except Exception as e:   # noqa: BLE001 -- the bench must not die on the optional path
                    why = f"{type(e).__name__}: {e}"
            box = [ident, why]
            dist.broadcast_object_list(box, src=0)   # every rank learns whether there is an id, so nobody waits alone
            ident, why = box
            if ident is not None:
                # ncclCommInitRank is itself a rendezvous of all ranks: it runs in a helper thread with a deadline, on a
                # context nothing else ever touches -- a rank whose helper is still inside RCCL after the deadline leaves
                # that context alone, takes the fall-back with the others and ends the process with os._exit
                import threading

                made = {}

                def _make():
                    try:
                        cctx = capi.Context(local_rank)
                        c = capi.ShardComm(cctx, rank, world, ident)
                        # a first all-gather of the size the run will do, under the deadline and outside the clock
                        trial = c.allgather_boundaries([(np.eye(3), np.full(3, float(rank)))] * M)
                        if len(trial) != M * world or any(abs(float(trial[r * M][1][0]) - r) > 0 for r in range(world)):
                            raise RuntimeError("trial all-gather returned the wrong boundaries")
                        made["comm"] = c
                    except Exception as e:   # noqa: BLE001
                        made["err"] = f"{type(e).__name__}: {e}"

                th = threading.Thread(target=_make, daemon=True)
                th.start()
                th.join(timeout=float(os.environ.get("SVO_BENCH_COMM_DEADLINE_S", "120")))
                if "comm" in made:
                    comm = made["comm"]
                else:
                    why = made.get("err", "ncclCommInitRank / the trial all-gather did not return before the deadline")
                    if th.is_alive():
                        comm_state["thread"] = th
        ok = torch.tensor([1 if comm is not None else 0])
        dist.all_reduce(ok, op=dist.ReduceOp.MIN)      # every rank takes the same path
        if int(ok.item()) == 1:
            return comm, None, f"ncclAllGather through svo_shard_allgather_boundaries (C ABI, librccl), {world} rank(s)"
        if comm is not None:
            comm.close()
            why = "another rank has no C-ABI communicator"
        group = None
        if not rehearsal:
            try:
                group = dist.new_group(backend="nccl")
                probe = torch.zeros(1, device=f"cuda:{local_rank}")
                dist.all_reduce(probe, group=group)
                torch.cuda.synchronize()
            except Exception as e:   # noqa: BLE001
                group = None
                why += f"; torch nccl group: {type(e).__name__}: {e}"
        ok = torch.tensor([1 if group is not None else 0])
        dist.all_reduce(ok, op=dist.ReduceOp.MIN)
        if int(ok.item()) == 1:
            return None, group, f"torch.distributed all_gather over nccl (C-ABI communicator unavailable: {why or 'no unique id'})"
        return None, None, f"torch.distributed all_gather over gloo (no RCCL communicator could be made: {why or 'no unique id'})"

    def single_chunk_leg():
        """ONE contiguous chunk per GPU (the north-star's partitioning), four streams, over rank 0's whole share --
        run while NO RCCL communicator exists in the process; then once more with device time stamps between the
        stages (svo_vo_set_stage_stamps), which say where a frame's time goes on this box."""
        out = {"single_chunk_comm_alive": False}
        try:   # an extra leg must not cost the run its line
            ctx1 = capi.Context(local_rank)
            one = capi.VisualOdometry(ctx1, W, H, C, seed=20261003, **vo_kw)
            one.init(lefts[0], rights[0])     # first use: streams, buffers and kernels of the pipeline come into being
            one.run_chunk(lefts[1:42], rights[1:42], pipeline=True)
            ctx1.sync()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            one.init(lefts[0], rights[0])
            rc, done, R1, t1, inl1, trk1, kf1 = one.run_chunk(lefts[1:], rights[1:], pipeline=True)
            ctx1.sync()
            dt = time.perf_counter() - t0
            if rc or done != share:
                out["single_chunk_frames_per_s"] = None
                out["single_chunk_note"] = f"tracking lost after {done} frames"
            else:
                out["t_seq"] = np.vstack([np.zeros((1, 3)), t1])
                out["single_chunk_frames_per_s"] = share / dt
                out["single_chunk_frames"] = share
                out["single_chunk_keyframe_rate"] = float(kf1.mean())
                n_st = min(share, 1000)
                one.set_stage_stamps(True)
                one.init(lefts[0], rights[0])
                t0 = time.perf_counter()
                rc2, done2, R2, t2, *_ = one.run_chunk(lefts[1:1 + n_st], rights[1:1 + n_st], pipeline=True)
                ctx1.sync()
                dt2 = time.perf_counter() - t0
                us, nfr = one.stage_us()
                one.set_stage_stamps(False)
                if rc2 == 0 and nfr > 0:
                    out["single_chunk_stage_us"] = dict(us, frames_averaged=nfr, frames_per_s_with_stamps=n_st / dt2,
                                                        bit_identical=bool(np.array_equal(t2, t1[:n_st])))
            one.close()
            ctx1.close()
        except Exception as e:   # noqa: BLE001
            out["single_chunk_error"] = f"{type(e).__name__}: {e}"
        return out

    def jobs_for(a: int, b: int, init: bool):
        """frames a+1 .. b of every chunk (chunk-local numbering), preceded by the seed frame a when
        the chunks initialise in this call"""
        lo = a if init else a + 1
        return [(v, lefts[s + lo:s + b + 1], rights[s + lo:s + b + 1]) for v, (s, e) in zip(sh.vos, bounds)]

    def run(a: int, b: int, init: bool, out, stats=None):
        """advance every chunk from its local frame a to b (init: seed on frame a first); -> capi.run_chunks' results"""
        res = capi.run_chunks(jobs_for(a, b, init), pipeline=pipeline, init=init)
        for m, (rc, done, Rs, ts, inl, trk, kf) in enumerate(res):
            if rc or done != b - a:
                raise SystemExit(f"bench: chunk {rank * M + m} lost tracking at local frame {a + done + 1} (rc {rc})")
            out[m].extend((Rs[i].copy(), ts[i].copy()) for i in range(done))
            if stats is not None:
                if m == 0 and os.environ.get("SVO_BENCH_DUMP_FRAMES"):  # per-frame record of chunk 0, for offline study
                    np.savez(os.environ["SVO_BENCH_DUMP_FRAMES"], inliers=inl, tracked=trk, keyframe=kf)
                stats["keyframes"] += int(kf.sum())
                stats["inliers"] += int(inl.sum())
                stats["tracked"] += int(trk.sum())
        return res

    def lk_launch_alone(sh_, frames_per_chunk: int):
        """Mean duration of a tracking launch that has the chip to ITSELF: the first lock-step group (one context, one
        stream) run alone over its chunks' first frames, HIP events on that stream.  -> (us per launch, launches,
        LK passes per launch)"""
        g0 = [(v, lefts[s:s + frames_per_chunk + 1], rights[s:s + frames_per_chunk + 1])
              for v, (s, e) in zip(sh_.vos[:G], bounds[:G])]
        capi.run_chunks(g0, pipeline=False, init=True)      # kernels of this shape loaded, buffers in being
        sh_.sync()
        c0 = sh_.ctxs[0]
        c0.enable_kernel_timing(True)
        c0.reset_kernel_time()
        res = capi.run_chunks(g0, pipeline=False, init=True)
        sh_.sync()
        ms, n = c0.kernel_time(capi.K_LK)
        c0.enable_kernel_timing(False)
        passes = sum(1 + len(r[6]) + int(r[6].sum()) for r in res)   # per chunk: the initialisation's stereo pass, one
        return (ms / max(n, 1) * 1e3, n, passes / max(n, 1))           # pass per frame, one stereo pass per keyframe

    def roofline_of(n_pts: int, lk_ms: float, lk_launches: int, passes: float, alone, elapsed_s: float, jobs_per_launch: int):
        """The tracking kernel against the HBM roofline the contract names (achieved / peak / frac, per launch with the
        chip to itself) and against the bound that binds it, vector-instruction issue (valu_*)."""
        per_launch = passes / max(lk_launches, 1)
        shared_s = lk_ms / max(lk_launches, 1) * 1e-3
        alone_us, alone_n, alone_passes = alone if alone else (None, 0, per_launch)
        bytes_alone = lk_algorithmic_bytes(n_pts) * alone_passes
        achieved = bytes_alone / (alone_us * 1e-6) / 1e9 if alone_us else None
        pmc = lk_pmc_constants(n_pts)
        roof = {
            "kernel": f"lk_track_kernel<3, {jobs_per_launch}>",
            "bound": "valu",
            "bound_note": "achieved / peak / frac price the kernel against the HBM roofline the contract names: algorithmic bytes "
                          "of a launch / the duration of a launch that has the chip to itself / 8 TB/s.  What binds the kernel is "
                          "vector-instruction issue: valu_frac = wave-instructions (SQ_INSTS_VALU) x the time one wave-instruction "
                          "of this kernel's mix costs a SIMD (tools/valu_rate.hip, same profiling session as the counters) / 1024 "
                          "SIMDs / launch duration",
            "achieved": achieved,
            "peak": 8000.0,
            "unit": "GB/s",
            "frac": achieved / 8000.0 if achieved is not None else None,
            "traffic": pmc["hbm_bytes_per_pass"] * alone_passes if pmc else None,
            "traffic_source": pmc["source"] if pmc else
                              f"null: {os.path.basename(LK_PMC_JSON.format(kpts=n_pts))} absent or taken on another lk.hip / keypoint count",
            "launch_alone_us": alone_us,
            "launch_alone_source": "HIP events on the stream of ONE lock-step group run alone in this invocation "
                                   f"({alone_n} launches): no other context's launches share the chip",
            "lk_passes_per_launch_alone": alone_passes,
            "algorithmic_bytes_per_launch": bytes_alone,
            "launch_shared_chip_us": shared_s * 1e6 if lk_launches else None,
            "launch_shared_chip_source": "HIP events on each context's stream in a SEPARATE instrumented pass over the timed "
                                         "frames; launches of several contexts overlap (not a denominator of frac)",
            "lk_passes_per_launch_shared": per_launch,
        }
        if pmc:
            ns = pmc["valu_ns_per_wave_inst"]
            need_s = pmc["valu_insts_per_pass"] * ns * 1e-9 / 1024.0       # per pass, all 1024 SIMDs issuing
            roof.update({
                "valu_insts_per_pass": pmc["valu_insts_per_pass"],
                "valu_ns_per_wave_inst": ns,
                "valu_cycles_per_wave_inst": pmc["valu_cycles_per_wave_inst"],
                "valu_clock_hz_in_kernel": pmc["valu_clock_hz_in_kernel"],
                "valu_issue_bound_us_per_launch_alone": need_s * alone_passes * 1e6,
                "valu_frac": need_s * alone_passes / (alone_us * 1e-6) if alone_us else None,
                "valu_chip_frac": need_s * passes / elapsed_s,
                "valu_note": pmc.get("valu_note"),
            })
        return roof

    ident = (np.eye(3), np.zeros(3))
    local = [[ident] for _ in range(M)]
    stats = {"keyframes": 0, "inliers": 0, "tracked": 0}

    trace("rendered; single-chunk leg")
    # ---- one chunk per GPU first (rank 0), while the process holds no RCCL communicator; then the communicator ----
    single = single_chunk_leg() if (rank == 0 and not args.no_extras) else {}
    if dist is not None:
        dist.barrier()
    comm, nccl_group, collective = make_communicator()
    coll = dict(dist=dist, comm=comm)
    if comm is None and nccl_group is not None:
        coll = dict(dist=dist, comm=None, group=nccl_group, device=f"cuda:{local_rank}")

    def exchange(loc):
        """the path's one exchange step: all-gather of the chunk-boundary poses"""
        if dist is None and comm is None:
            return [x[-1] for x in loc]
        return chunked.all_gather_chunk_boundaries(coll["dist"], [x[-1] for x in loc], device=coll.get("device", "cpu"),
                                                   comm=coll["comm"], group=coll.get("group"))

    def max_over_ranks(x: float) -> float:
        if dist is None:
            return x
        tt = torch.tensor([x], dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        return float(tt.item())

    trace("communicator made; timed region")
    # ---- the timed region: EXACTLY --steps steps + the path's one exchange, REPEATED (each repeat: every chunk's stereo
    # initialisation + its first W frames untimed, then the K timed steps) until at least --min-timed-s seconds are on the
    # clock, so that a box's +-2 % does not decide a round.  value = all frames of all repeats / all time.
    # A plain run (no --full) does it once.
    reps = []               # (elapsed max over ranks, elapsed local)
    local = None
    target_s = max(0.0, args.min_timed_s)
    n_reps = 1
    r_i = 0
    while r_i < n_reps:
        loc_r = [[ident] for _ in range(M)]
        st_r = {"keyframes": 0, "inliers": 0, "tracked": 0}
        run(0, Wn, True, loc_r)     # warm-up: every chunk's stereo initialisation + its first W frames (untimed)
        sh.sync()
        for c in sh.ctxs:
            c.enable_kernel_timing(False)   # the timed region carries NO event records
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()
        sh.sync()
        t0 = time.perf_counter()
        res_timed = run(Wn, L, False, loc_r, st_r)
        boundaries = exchange(loc_r)
        starts = chunked.prefix_transforms(boundaries)  # global pose of every chunk's first frame
        assert len(starts) == world * M
        sh.sync()
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        el_local = time.perf_counter() - t0
        el = max_over_ranks(el_local)
        reps.append((el, el_local))
        if local is None:
            local, stats = loc_r, st_r
            n_reps = max(1, min(args.max_repeats, int(np.ceil(target_s / max(el, 1e-6)))))   # every rank: the same number
        elif not all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for la, lb in zip(local, loc_r) for a, b in zip(la, lb)):
            raise SystemExit(f"bench: repeat {r_i} of the timed region did not reproduce the first one bit for bit")
        r_i += 1
    elapsed = sum(e for e, _ in reps) / len(reps)           # mean duration of the K timed steps
    elapsed_local = sum(e for _, e in reps) / len(reps)
    ranks_seen = dist.get_world_size() if dist is not None else 1   # after a real all-gather over the group
    if args.dump_outputs and rank == 0:
        # the last timed step as run_chunks handed it to its caller (rank 0's chunks), and the exchange's result
        dump = {"last_step_R": [r[2][-1] for r in res_timed], "last_step_t": [r[3][-1] for r in res_timed],
                "last_step_inliers": [r[4][-1] for r in res_timed], "last_step_tracked": [r[5][-1] for r in res_timed],
                "last_step_keyframe": [r[6][-1] for r in res_timed],
                "chunk_start_R": [R for R, _ in starts], "chunk_start_t": [t for _, t in starts]}
        os.makedirs(args.dump_outputs, exist_ok=True)
        for name, a in dump.items():
            np.save(os.path.join(args.dump_outputs, f"{name}.npy"), np.asarray(a, np.float64))

    trace("instrumented pass")
    # ---- the SAME frames once more with HIP events around every launch: per-kernel launch durations for the
    # roofline object and the stage table, and what the event records cost (elapsed_events / elapsed) ----
    times = {}
    elapsed_events = None
    if not args.no_kernel_timing:
        local_ev = [[ident] for _ in range(M)]
        run(0, Wn, True, local_ev)
        sh.sync()
        for c in sh.ctxs:
            c.enable_kernel_timing(True)
            c.reset_kernel_time()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()
        sh.sync()
        t0 = time.perf_counter()
        run(Wn, L, False, local_ev)
        sh.sync()
        torch.cuda.synchronize()
        elapsed_events = time.perf_counter() - t0
        for name, kid in (("pyramid", capi.K_PYRAMID), ("lk", capi.K_LK), ("fransac", capi.K_FRANSAC),
                          ("triangulate", capi.K_TRIANGULATE), ("pnp", capi.K_PNP), ("anms", capi.K_ANMS)):
            per = [c.kernel_time(kid) for c in sh.ctxs]
            times[name] = (sum(p[0] for p in per), sum(p[1] for p in per))
        for c in sh.ctxs:
            c.enable_kernel_timing(False)
        same = all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
                   for la, lb in zip(local, local_ev) for a, b in zip(la, lb))
        if not same:
            raise SystemExit("bench: the instrumented pass did not reproduce the timed pass bit for bit")
    n_frames = K * M
    alone_main = None
    if not args.no_kernel_timing and M > 1:
        try:
            alone_main = lk_launch_alone(sh, min(L, 12))
        except Exception:   # noqa: BLE001 -- an extra leg must not cost the run its line
            alone_main = None

    trace("second timed figure")
    # ---- second timed figure: the whole share again, chunk initialisations inside the clock ----
    extras = {}
    local2 = None
    if not args.no_extras:
        local2 = [[ident] for _ in range(M)]
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(0, L, True, local2)
        exchange(local2)
        sh.sync()
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        t_full = max_over_ranks(time.perf_counter() - t0)
        extras["value_including_chunk_inits"] = world * share / t_full
        extras["rerun_bit_identical"] = all(
            np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
            for la, lb in zip(local, local2) for a, b in zip(la, lb))

    # ---- stitch: rebase with the prefix transforms, gather the trajectories (configs[3]) ----
    mine = chunked.join_chunks(local, starts[rank * M:(rank + 1) * M])
    if dist is not None:
        parts = chunked.gather_trajectories(dist, mine, device="cpu", counts=[share + 1] * world, as_array=True)
        traj = chunked.array_to_poses(np.concatenate([parts[0]] + [p[1:] for p in parts[1:]]))   # ONE tensor collective
    else:
        traj = mine

    result = None
    if rank == 0:
        truth = rel_truth(poses_all)
        t_truth = np.array([t for _, t in truth])
        t_sh = np.array([t for _, t in traj])
        path_len = float(np.sum(np.linalg.norm(np.diff(t_truth, axis=0), axis=1)))
        fps = world * n_frames / elapsed
        kf_rate = stats["keyframes"] / n_frames
        ate_sh = chunked.ate_rmse(t_sh, t_truth)
        result = {
            "metric": f"stereo frames/sec @1241x376, {n_kpts} kpts",
            "value": fps,
            "unit": "frames/s",
            "n_gpus": world,
            "ranks_seen": ranks_seen,
            "steps": K,
            "warmup": Wn,
            "ms_per_step": elapsed / K * 1e3,
            "repeats": len(reps),
            "timed_s_total": sum(e for e, _ in reps),
            "value_per_repeat": [world * n_frames / e for e, _ in reps],
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "u8/i32 fixed-point (LK) + f32/f64 (geometry)",
            "data": "synthetic",
            "config": {
                "workload": f"synthetic loop stream 1241x376x3 (0.9 m/frame, 492-frame lap), {world * share + 1} frames, "
                            f"grid step {grid_step} -> ANMS {n_kpts} keypoints, front-end only (BASELINE configs[1]): "
                            "pyramid + LK + F-RANSAC + PnP-RANSAC + keyframe path (LK L->R, F-RANSAC, DLT triangulation)",
                "keyframe_min_inliers": kf_min,
                "parallelism": f"{M} contiguous chunk(s) of {L} frames per GPU x{world} GPU(s), one all-gather of "
                               "chunk-boundary poses",
                "collective": collective,
                # where an RCCL communicator was alive in the process (it holds hardware queues)
                "comm_alive_during": {"timed_region": bool(comm is not None or nccl_group is not None),
                                      "single_chunk_leg": False},
                "chunks_per_gpu": M,
                "chunks_per_context": G,
                "frames_per_chunk": L,
                "pipeline": "four HIP streams per chunk: filters + tracking pass from the tracked set | PnP, decision, refinement, "
                            "keyframe hand-over | stereo path two frames ahead | pyramids, triangulation, tracking pass from the "
                            "keyframe candidate, ahead" if pipeline
                            else "one in-order HIP stream per context",
                "keyframe_rate": kf_rate,
                "frames_per_step": M * world,
                "mean_tracked": stats["tracked"] / n_frames,
                "mean_pnp_inliers": stats["inliers"] / n_frames,
                "render_s": render_s,
                "stage_ms_per_frame": {k: v[0] / n_frames for k, v in times.items()},
                "stage_ms_source": "instrumented pass (HIP events), not the timed region",
            },
            "event_records": {
                "timed_region": "none",
                "value_with_event_records": (world * n_frames / elapsed_events) if elapsed_events else None,
                "cost_frac": (elapsed_events / elapsed_local - 1.0) if elapsed_events else None,
                "note": "the instrumented pass is rank-local (no collective inside its clock)",
            },
            "path_length_m": path_len,
            "ate_rmse_vs_truth": ate_sh,
            "ate_over_path_length": ate_sh / path_len,
        }
        if args.full:
            lk_ms, lk_launches = times.get("lk", (0.0, 0))
            if not lk_launches and M > 1:
                # no instrumented pass: a lock-step group step queues two tracking launches per context (the frame's pass of
                # all its chunks, the stereo pass of those that keyframe)
                lk_launches = 2 * K * len(sh.ctxs)
            # passes carried by the LK launches of the timed region: one tracking pass per frame + one stereo pass per keyframe
            passes = n_frames + stats["keyframes"]
            roof = roofline_of(n_kpts, lk_ms, lk_launches, passes, alone_main, elapsed, G if M > 1 else 1)
            roof["launches_per_step"] = lk_launches / K
            roof["frame_hbm_frac"] = frame_algorithmic_bytes(n_kpts, kf_rate) / (elapsed / n_frames) / 8e12
            result["roofline"] = roof
        result.update(extras)

    # ---- one contiguous chunk per GPU: measured before the communicator existed (single); its trajectory figures ----
    if rank == 0 and single:
        result.update({k: v for k, v in single.items() if k != "t_seq"})
        if "t_seq" in single:
            t_seq = single["t_seq"]
            n1 = share + 1
            result["ate_rmse_sequential_vs_truth"] = chunked.ate_rmse(t_seq, t_truth[:n1])
            result["ate_rmse_sharded_vs_sequential"] = chunked.ate_rmse(t_sh[:n1], t_seq)
            result["ate_rmse_sharded_vs_truth_same_frames"] = chunked.ate_rmse(t_sh[:n1], t_truth[:n1])
            result["ate_sharded_vs_sequential_over_path_length"] = (
                result["ate_rmse_sharded_vs_sequential"] / (path_len * share / (world * share)))

    trace("legs: vocabulary")
    # ================= the legs beyond the front-end's own clock =================
    def orb_features(ctxf, first: int, count: int):
        """ORB features (cv::ORB's own shape: 8 levels x 1.2, the detector's default) of this rank's left images
        [first, first + count): 32 images per set of launches (svo_orb_extract_batch).  -> n [count], xy, desc"""
        fn = np.zeros(count, np.int32)
        fxy, fdesc = np.empty((count, 500, 2), np.float32), np.empty((count, 500, 8), np.uint32)
        imgs = lefts[first:first + count]
        for a in range(0, count, 256):   # 32 images per set of launches, eight sets per call (one read-back per call)
            b = min(count, a + 256)
            ctxf.orb_extract_batch_padded(imgs[a:b], out=(fn[a:b], fxy[a:b], fdesc[a:b]))
        return fn, fxy, fdesc

    def all_ranks_ok(ok: bool) -> bool:
        return max_over_ranks(0.0 if ok else 1.0) == 0.0

    legs = {}
    voc = None
    want_detector = not args.no_extras and not args.no_detector
    if want_detector:
        # the vocabulary exists BEFORE any clock starts, as the reference's does (it loads orb_voc00.yml.gz at start-up,
        # include/visualSLAM.h:131-134): k 9, L 6 (src/bagOfWordsDetector.cpp:46-56), trained on the GPU on every fourth
        # frame of the first lap (rank 0 holds those frames: a rank's share is longer than a lap in every driver run)
        try:
            if rank == 0:
                ctxv = capi.Context(local_rank)
                t0 = time.perf_counter()
                n_train = min(share + 1, 492)
                tn, txy, tdesc = orb_features(ctxv, 0, n_train)
                train = [tdesc[i, :tn[i]] for i in range(0, n_train, 4)]
                voc = capi.Vocabulary.train(ctxv, train, k=9, L=6, seed=20261003)
                legs["vocabulary"] = {"k": voc.k, "L": voc.L, "nodes": voc.n_nodes, "words": voc.n_words, "training_images": len(train),
                                      "features_and_training_s": time.perf_counter() - t0, "inside_a_clock": False}
        except Exception as e:   # noqa: BLE001
            voc = None
            legs["vocabulary_error"] = f"{type(e).__name__}: {e}"
        want_detector = all_ranks_ok(rank != 0 or voc is not None)

    trace("leg: end to end")
    # ---- configs[3] END TO END in one clock: chunk-sharded front-end incl. every chunk's initialisation ->
    # the all-gather of chunk-boundary poses -> stitched trajectory on rank 0 -> ORB features on every rank's own frames ->
    # all-gather of the features -> THE DETECTOR SHARDED LIKE THE FRONT-END (chunked.sharded_detect: every rank fills its
    # database with the frames before its share as entries that are not queries, queries its own share after a warm-up of
    # the temporal window; the verdicts are those of one detector over the whole stream: tests/test_chunked.py,
    # tests/test_gpu_bow.py) -> the verdicts gathered on rank 0, gated as the reference gates them -> ONE global solve.
    # Rank-local failures never skip a collective.
    e2e_closures, e2e_traj = None, None
    if want_detector:
        fail = None
        n_all = world * share + 1
        q_shares = chunked.detect_shares(n_all, world)
        mine_n = share + (1 if rank == world - 1 else 0)       # the overlap frame belongs to the next rank
        try:
            # the vocabulary on every rank (rank 0 trained it; 3.5 MB of arrays over the control group), outside the clock
            box = [None]
            if rank == 0:
                va = voc.arrays()
                box = [(voc.k, voc.L, va["parent"], va["desc"], va["weight"])]
            if dist is not None:
                dist.broadcast_object_list(box, src=0)
            ctxf = capi.Context(local_rank)
            ctxd = capi.Context(local_rank)
            voc_r = voc if rank == 0 else capi.Vocabulary.from_arrays(ctxd, *box[0])
            det = capi.LoopDetector(ctxd, W, H, C, seed=5, max_entries=n_all + 9)
            det.set_vocabulary(voc_r, 2)
            if rank == 0:
                ctxg = capi.Context(local_rank)
            orb_features(ctxf, 0, min(mine_n, 256))                # buffers of the extractor (and the wrapper's pinned block) come into being
        except Exception as e:   # noqa: BLE001
            fail = f"{type(e).__name__}: {e}"
        if all_ranks_ok(fail is None):
            if dist is not None:
                dist.barrier()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            T = {}
            loc3 = [[ident] for _ in range(M)]
            try:
                run(0, L, True, loc3)
                sh.sync()
            except (Exception, SystemExit) as e:   # noqa: BLE001
                fail = f"front-end: {type(e).__name__}: {e}"
                loc3 = [[ident] * (L + 1) for _ in range(M)]
            T["front_end"] = time.perf_counter() - t0
            starts3 = chunked.prefix_transforms(exchange(loc3))
            mine3 = chunked.join_chunks(loc3, starts3[rank * M:(rank + 1) * M])
            if dist is not None:
                parts = chunked.gather_trajectories(dist, mine3, device="cpu", counts=[share + 1] * world, as_array=True)
                traj3 = chunked.array_to_poses(np.concatenate([parts[0]] + [p_[1:] for p_ in parts[1:]]))
            else:
                traj3 = mine3
            T["exchange_and_stitch"] = time.perf_counter() - t0 - T["front_end"]
            t1 = time.perf_counter()
            try:
                fn, fxy, fdesc = orb_features(ctxf, 0, mine_n)
            except Exception as e:   # noqa: BLE001
                fail = fail or f"features: {type(e).__name__}: {e}"
                fn, fxy, fdesc = np.zeros(mine_n, np.int32), np.zeros((mine_n, 500, 2), np.float32), np.zeros((mine_n, 500, 8), np.uint32)
            T["features"] = time.perf_counter() - t1
            t1 = time.perf_counter()
            if dist is not None:
                # over the library's RCCL communicator when the run has one (the C-ABI path of the boundary all-gather), else
                # over the control group
                an, axy, adesc = chunked.all_gather_frame_features(dist, fn, fxy, fdesc, comm=comm,
                                                                   counts=[share + (1 if r == world - 1 else 0) for r in range(world)])
            else:
                an, axy, adesc = fn, fxy, fdesc
            T["feature_all_gather"] = time.perf_counter() - t1
            t1 = time.perf_counter()
            q_lo, q_hi = q_shares[rank]
            mine_v = []
            try:
                assert len(an) == n_all
                mine_v = chunked.sharded_detect(lambda a_, b_: det.fill_features_batch(an[a_:b_], axy[a_:b_], adesc[a_:b_]),
                                                lambda a_, b_: det.submit_features_batch(an[a_:b_], axy[a_:b_], adesc[a_:b_]),
                                                det.collect, q_lo, q_hi, collect_many=det.collect_batch)
            except Exception as e:   # noqa: BLE001
                fail = fail or f"detector: {type(e).__name__}: {e}"
                mine_v = [dict(status=1, match=-1, query=q_lo + i) for i in range(q_hi - q_lo)]
            T["detector_own_share"] = time.perf_counter() - t1
            t1 = time.perf_counter()
            verdicts = chunked.gather_verdicts(dist, mine_v, q_shares) if dist is not None else mine_v
            T["verdict_gather"] = time.perf_counter() - t1
            if rank == 0:
                try:
                    t1 = time.perf_counter()
                    e2e_closures = chunked.gate_closures([v["match"] if v["status"] == 0 and v["match"] >= 1 else -1 for v in verdicts])
                    pg3 = capi.PoseGraph(ctxg)
                    est3, chi3 = chunked.global_solve(pg3, traj3, e2e_closures, iters=10)
                    pg3.close()
                    T["gate_and_global_solve"] = time.perf_counter() - t1
                    e2e_traj = (traj3, est3, verdicts)
                except Exception as e:   # noqa: BLE001
                    fail = fail or f"solve: {type(e).__name__}: {e}"
            if dist is not None:
                dist.barrier()
            t_e2e = max_over_ranks(time.perf_counter() - t0)
            ok = all_ranks_ok(fail is None)
            if rank == 0:
                if ok:
                    legs["end_to_end"] = {
                        "what": "BASELINE configs[3] in ONE clock: chunk-sharded front-end incl. every chunk's initialisation, the "
                                "all-gather of chunk-boundary poses, the stitched trajectory on rank 0, ORB (cv::ORB's shape, 32 images per "
                                "set of launches) on every rank's own frames, the all-gather of 20 KB per frame, the DETECTOR SHARDED LIKE THE "
                                "FRONT-END (every rank: the frames before its share enter its database without being queries, its share is "
                                "scored and judged after 8 warm-up frames; vocabulary mode, 16 frames per set of launches), the verdicts "
                                "gathered on rank 0, the reference's gating, ONE global solve of 10 Gauss-Newton iterations",
                        "end_to_end_s": t_e2e, "frames": world * share, "end_to_end_frames_per_s": world * share / t_e2e,
                        "feature_all_gather_over": "ncclAllGather through svo_shard_allgather_bytes" if comm is not None else
                                                   ("nothing to gather (one rank)" if dist is None else "gloo (control group)"),
                        "rank0_stage_s": T, "serial_tail_on_rank0_s": T.get("gate_and_global_solve", 0.0),
                        "detector_queries_per_rank": [e_ - s_ for s_, e_ in q_shares],
                        "closures": len(e2e_closures), "detections": int(sum(v["status"] == 0 for v in verdicts))}
                else:
                    legs["end_to_end_error"] = fail or "another rank failed"
        elif rank == 0:
            legs["end_to_end_error"] = fail or "another rank could not make its contexts"
        try:
            det.close()
            if rank != 0:
                voc_r.close()
            ctxd.close()
            if rank == 0:
                ctxg.close()
            ctxf.close()
        except Exception:   # noqa: BLE001
            pass

    trace("leg: configs2")
    # ---- configs[2] END TO END on one GPU: the front-end of the whole share (64 chunks, initialisations
    # included) WHILE the detector takes the same left images on a context of its own (ORB + scoring, 16 frames per set of
    # launches) and its verdicts are collected; then the in-loop solves: an optimisation of 10 iterations at EVERY closure,
    # the later odometry re-anchored on the optimised pose as the reference does (src/VisualSLAM.cpp:76-86).  Rank 0.
    if want_detector and rank == 0:
        try:
            import threading

            from scipy.spatial.transform import Rotation as _Rot

            if os.environ.get("SVO_BENCH_DET_PRIORITY"):
                os.environ["SVO_CTX_PRIORITY_EXPERIMENT"] = os.environ["SVO_BENCH_DET_PRIORITY"]
            ctxd = capi.Context(local_rank)
            os.environ.pop("SVO_CTX_PRIORITY_EXPERIMENT", None)
            det = capi.LoopDetector(ctxd, W, H, C, seed=5, max_entries=share + 9)
            det.set_vocabulary(voc, 2)
            frames_l = [lefts[i] for i in range(share + 1)]
            det.submit_batch(frames_l[:16])                      # first use: the extractor's kernels and buffers
            for _ in range(16):
                det.collect()
            det.close()
            det = capi.LoopDetector(ctxd, W, H, C, seed=5, max_entries=share + 9)
            det.set_vocabulary(voc, 2)
            ctxg = capi.Context(local_rank)
            box = {}

            def front_end():
                try:
                    loc = [[ident] for _ in range(M)]
                    run(0, L, True, loc)
                    sh.sync()
                    box["loc"] = loc
                    box["fe_s"] = time.perf_counter() - t0
                except (Exception, SystemExit) as e:   # noqa: BLE001
                    box["fe_error"] = f"{type(e).__name__}: {e}"

            def detector():
                try:
                    det.submit_batch(frames_l)
                    box["det_submitted_s"] = time.perf_counter() - t0
                    box["submitted_event"].set()
                    box["verdicts"] = []
                    while len(box["verdicts"]) < len(frames_l):
                        box["verdicts"] += det.collect_batch(min(64, len(frames_l) - len(box["verdicts"])))
                        if len(box["verdicts"]) <= 64:
                            box["det_first_verdicts_s"] = time.perf_counter() - t0
                    box["det_s"] = time.perf_counter() - t0
                except Exception as e:   # noqa: BLE001
                    box["det_error"] = f"{type(e).__name__}: {e}"
                    box["submitted_event"].set()

            torch.cuda.synchronize()
            t0 = time.perf_counter()
            th = [threading.Thread(target=front_end), threading.Thread(target=detector)]
            submitted = threading.Event()
            box["submitted_event"] = submitted
            if os.environ.get("SVO_BENCH_C2_SEQUENTIAL"):
                for x in th:
                    x.start()
                    x.join()
            else:
                # the detector's frames are queued FIRST (3 ms of host time alone): started together, the two threads' HIP
                # calls take turns on the runtime's locks and the detector's 1 300 launches trickle out over the front-end's
                # whole enqueue (137 ms, measured) -- its kernels were never on the device to share it
                th[1].start()
                if not os.environ.get("SVO_BENCH_C2_TOGETHER"):
                    submitted.wait(timeout=60)
                th[0].start()
                for x in th:
                    x.join()
            t_overlap = time.perf_counter() - t0
            if "loc" not in box or "verdicts" not in box:
                raise RuntimeError(box.get("fe_error") or box.get("det_error") or "a leg did not finish")
            traj2 = chunked.join_chunks(box["loc"], chunked.prefix_transforms([x[-1] for x in box["loc"]]))
            cl2 = chunked.gate_closures([v["match"] if v["status"] == 0 and v["match"] >= 1 else -1 for v in box["verdicts"]])
            pg2c = capi.PoseGraph(ctxg)
            Rc, tc = np.eye(3), np.zeros(3)          # the re-anchoring transform since the last closure
            n_solves = 0
            # frame by frame in effect (a closure's edge before its vertex, the solve right after it), but the vertices between
            # two closures are staged in one call: they are the raw poses under ONE re-anchoring transform
            R_all = np.array([np.asarray(p_[0], np.float64) for p_ in traj2])
            t_all_ = np.array([np.asarray(p_[1], np.float64).reshape(3) for p_ in traj2])
            stops = sorted(q for q in cl2 if 1 <= q < len(traj2)) + [len(traj2)]
            q0 = 1
            for stop in stops:
                q1 = min(stop + 1, len(traj2))       # the segment ends WITH the closure's vertex
                if q1 > q0:
                    seg = list(zip(Rc @ R_all[q0:q1], t_all_[q0:q1] @ Rc.T + tc))
                    lc = np.full(q1 - q0, -1, np.int32)
                    if stop < len(traj2):
                        lc[stop - q0] = max(cl2[stop] - 1, 0)
                    pg2c.augment_nodes(chunked.poses7(seg), lc)
                if stop < len(traj2):
                    pg2c.optimize(10)
                    n_solves += 1
                    e7 = pg2c.estimates()[stop]
                    Ro = _Rot.from_quat(e7[3:]).as_matrix()
                    # optimised pose of q = C * raw pose of q  ->  C = opt * raw^-1
                    Rr, tr = traj2[stop]
                    Rc = Ro @ Rr.T
                    tc = e7[:3] - Rc @ tr
                q0 = q1
            est2 = pg2c.estimates()
            t_all = time.perf_counter() - t0
            pg2c.close()
            legs["configs2"] = {
                "what": "BASELINE configs[2] end to end on one GPU: the front-end over the whole share (64 chunks, their stereo "
                        "initialisations included) WHILE the detector's context extracts ORB and scores the same left images (16 per set of "
                        "launches) and its verdicts are collected; then the graph built frame by frame with an optimisation of 10 "
                        "iterations at EVERY closure and the later odometry re-anchored (src/VisualSLAM.cpp:76-86)",
                "frames": share, "configs2_frames_per_s": share / t_all, "wall_s": t_all,
                "front_end_and_detector_side_by_side_s": t_overlap, "front_end_done_s": box.get("fe_s"), "detector_done_s": box.get("det_s"),
                "detector_submitted_s": box.get("det_submitted_s"), "detector_first_64_verdicts_s": box.get("det_first_verdicts_s"),
                "in_loop_solves": n_solves,
                "in_loop_solves_s": t_all - t_overlap, "closures": len(cl2),
                "ate_rmse_vs_truth_m": chunked.ate_rmse(est2[:, :3], np.array([t for _, t in rel_truth(poses_all)])[:share + 1])}
            det.close()
            ctxd.close()
            ctxg.close()
        except Exception as e:   # noqa: BLE001
            legs["configs2_error"] = f"{type(e).__name__}: {e}"

    trace("leg: host images")
    # ---- the headline's timed region with the frames in PINNED HOST memory (KITTI replay is host images):
    # the library uploads every lock-step group's step f + 2 on a copy stream of the group's context while step f computes
    # (frontend.hip: chain_enqueue).  Every rank takes part; no collective inside the clock but the barriers around it.
    if not args.no_extras and not args.no_host_images and M > 1:
        fail = None
        try:
            t0 = time.perf_counter()
            # ONE pinned allocation per side (3 202 separate pin_memory() calls took 9 s on one rank and did not finish in minutes
            # when four processes made them at once: every hipHostMalloc maps its pages for the GPUs under a driver lock)
            pin_l = torch.empty((share + 1, H, W, C), dtype=torch.uint8, pin_memory=True)
            pin_r = torch.empty((share + 1, H, W, C), dtype=torch.uint8, pin_memory=True)
            for i in range(share + 1):
                pin_l[i].copy_(lefts[i], non_blocking=True)
                pin_r[i].copy_(rights[i], non_blocking=True)
            torch.cuda.synchronize()
            hl = [pin_l[i] for i in range(share + 1)]
            hr = [pin_r[i] for i in range(share + 1)]
            t_pin = time.perf_counter() - t0
            trace(f"host images: pinned {share + 1} frame pairs in {t_pin:.1f} s")

            def run_host(a: int, b: int, init: bool, out=None):
                lo = a if init else a + 1
                jobs = [(v, hl[s0 + lo:s0 + b + 1], hr[s0 + lo:s0 + b + 1]) for v, (s0, e0) in zip(sh.vos, bounds)]
                res = capi.run_chunks(jobs, pipeline=False, init=init)
                for m_, (rc, done, Rs, ts, inl, trk, kf) in enumerate(res):
                    if rc or done != b - a:
                        raise RuntimeError(f"host-image leg: chunk {rank * M + m_} stopped at local frame {a + done + 1} (rc {rc})")
                    if out is not None:
                        out.append(ts[-1].copy())
            run_host(0, Wn, True)
            sh.sync()
            trace("host images: first run through the upload ring done")
        except Exception as e:   # noqa: BLE001
            fail = f"{type(e).__name__}: {e}"
        if all_ranks_ok(fail is None):
            reps_h, last_h = [], []
            for _ in range(max(1, min(len(reps), 4))):
                try:
                    run_host(0, Wn, True)
                    sh.sync()
                    if dist is not None:
                        dist.barrier()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    last_h = []
                    run_host(Wn, L, False, last_h)
                    sh.sync()
                    torch.cuda.synchronize()
                    el_h = time.perf_counter() - t0
                except Exception as e:   # noqa: BLE001
                    fail, el_h = f"{type(e).__name__}: {e}", 0.0
                    if dist is not None:
                        dist.barrier()
                reps_h.append(max_over_ranks(el_h))
            ok = all_ranks_ok(fail is None)
            if rank == 0:
                if ok:
                    el = sum(reps_h) / len(reps_h)
                    same_h = all(np.array_equal(a_, b_[-1][1]) for a_, b_ in zip(last_h, local))
                    legs["host_images"] = {
                        "value_host_images": world * n_frames / el, "unit": "frames/s", "ms_per_step": el / K * 1e3, "repeats": len(reps_h),
                        "h2d_GB_per_s_per_gpu": n_frames * 2 * W * H * C / el / 1e9,
                        "what": "the headline's K timed steps with every frame in pinned host memory: each lock-step group's context "
                                "uploads step f + 2 (the left and right images of its 16 chunks) on a copy stream of its own while step f "
                                "computes, a ring of three device slots",
                        "poses_equal_the_resident_run": bool(same_h), "pin_memory_s": t_pin}
                else:
                    legs["host_images_error"] = fail or "another rank failed"
        elif rank == 0:
            legs["host_images_error"] = fail or "another rank failed before the clock"
        hl = hr = pin_l = pin_r = None

    trace("leg: kpts8192")
    # ---- configs[4]'s shape in the SAME invocation (VERDICT r4 #1c): 8192 keypoints per frame (grid step 7 -> 9152 lattice
    # points -> ANMS 8192, keyframe rule 4000) over the same frames, the same chunking, every rank taking part ----
    if args.kpts == 4096 and not args.no_extras and not args.no_kpts8192:
        sub = None
        sh.close()      # the headline's contexts give their hardware queues back before another set of four is made
        sh = None
        try:
            kw8 = dict(grid_step=7, anms_keep=8192, keyframe_min_inliers=4000)
            sh8 = chunked.ShardedVO(capi, local_rank, W, H, C, M, G, first_chunk_id=rank * M, seed=20261003, **kw8)

            def run8(a: int, b: int, init: bool, st=None):
                lo = a if init else a + 1
                jobs = [(v, lefts[s0 + lo:s0 + b + 1], rights[s0 + lo:s0 + b + 1]) for v, (s0, e0) in zip(sh8.vos, bounds)]
                res = capi.run_chunks(jobs, pipeline=pipeline, init=init)
                for m, (rc, done, Rs, ts, inl, trk, kf) in enumerate(res):
                    if rc or done != b - a:
                        raise RuntimeError(f"8192-keypoint leg: chunk {rank * M + m} lost tracking at local frame {a + done + 1} (rc {rc})")
                    if st is not None:
                        st["keyframes"] += int(kf.sum())
                        st["inliers"] += int(inl.sum())
                        st["tracked"] += int(trk.sum())
                        st["t_last"].append(ts[-1].copy())
            reps8, first8, st8 = [], None, None
            n_reps8, r_i = 1, 0
            while r_i < n_reps8:
                st_r = {"keyframes": 0, "inliers": 0, "tracked": 0, "t_last": []}
                run8(0, Wn, True)
                sh8.sync()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run8(Wn, L, False, st_r)
                sh8.sync()
                torch.cuda.synchronize()
                reps8.append(time.perf_counter() - t0)      # rank-local: this leg has no collective inside its clock
                if first8 is None:
                    first8, st8 = st_r["t_last"], st_r
                    n_reps8 = max(1, min(args.max_repeats, int(np.ceil(0.5 * target_s / max(reps8[0], 1e-6)))))
                elif not all(np.array_equal(a, b) for a, b in zip(first8, st_r["t_last"])):
                    raise RuntimeError(f"8192-keypoint leg: repeat {r_i} did not reproduce the first one bit for bit")
                r_i += 1
            el8_local = sum(reps8) / len(reps8)
            # the same frames with HIP events around every launch (shared-chip durations), then one group alone
            run8(0, Wn, True)
            sh8.sync()
            for c in sh8.ctxs:
                c.enable_kernel_timing(True)
                c.reset_kernel_time()
            run8(Wn, L, False)
            sh8.sync()
            per = [c.kernel_time(capi.K_LK) for c in sh8.ctxs]
            for c in sh8.ctxs:
                c.enable_kernel_timing(False)
            lk_ms8, lk_n8 = sum(p_[0] for p_ in per), sum(p_[1] for p_ in per)
            alone8 = lk_launch_alone(sh8, min(L, 12)) if M > 1 else None
            sh8.close()
            leg_ok = True
        except Exception as e:   # noqa: BLE001 -- an extra leg must not cost the run its line
            leg_ok, sub = False, {"error": f"{type(e).__name__}: {e}"}
        # every rank reaches these two collectives whatever happened above (no rank may wait alone)
        el8 = max_over_ranks(el8_local if leg_ok else 0.0)
        all_ok = max_over_ranks(0.0 if leg_ok else 1.0) == 0.0
        try:
            if rank == 0 and leg_ok and not all_ok:
                sub = {"error": "the 8192-keypoint leg failed on another rank"}
            if rank == 0 and all_ok:
                nf8 = K * M
                sub = {"metric": "stereo frames/sec @1241x376, 8192 kpts", "value": world * nf8 / el8, "unit": "frames/s",
                       "ms_per_step": el8 / K * 1e3, "repeats": len(reps8), "value_per_repeat": [world * nf8 / e for e in reps8],
                       "rerun_bit_identical": True,
                       "workload": "the same frames and chunking as the headline; grid step 7 -> 9152 lattice points -> ANMS 8192 "
                                   "keypoints, keyframe rule 4000 (BASELINE configs[4]'s shape)",
                       "keyframe_rate": st8["keyframes"] / nf8, "mean_tracked": st8["tracked"] / nf8,
                       "mean_pnp_inliers": st8["inliers"] / nf8,
                       "roofline": roofline_of(8192, lk_ms8, lk_n8, nf8 + st8["keyframes"], alone8, el8, G if M > 1 else 1)}
            # one chunk per GPU at 8192 keypoints (rank 0, four streams), over the first frames of the share
            if rank == 0 and all_ok:
                n1 = min(share, 400)
                ctx8 = capi.Context(local_rank)
                one8 = capi.VisualOdometry(ctx8, W, H, C, seed=20261003, **kw8)
                one8.init(lefts[0], rights[0])
                one8.run_chunk(lefts[1:42], rights[1:42], pipeline=True)
                ctx8.sync()
                t0 = time.perf_counter()
                one8.init(lefts[0], rights[0])
                rc8, done8, *_ = one8.run_chunk(lefts[1:1 + n1], rights[1:1 + n1], pipeline=True)
                ctx8.sync()
                dt8 = time.perf_counter() - t0
                sub["single_chunk_frames_per_s"] = n1 / dt8 if (rc8 == 0 and done8 == n1) else None
                sub["single_chunk_frames"] = n1
                one8.close()
                ctx8.close()
        except Exception as e:   # noqa: BLE001 -- an extra leg must not cost the run its line
            sub = {"error": f"{type(e).__name__}: {e}"}
        if rank == 0 and result is not None:
            result["kpts8192"] = sub
    if rank == 0 and result is not None:
        result.update(legs)

    trace("leg: pose graph")
    # ---- configs[3]'s global solve on the stitched trajectory (rank 0; also configs[2]'s figure) ----
    if rank == 0 and not args.no_extras:
        try:   # an extra leg must not cost the run its line
            matches = synth.loop_closures(poses_all, max_dist=0.3, max_angle_deg=10.0, min_gap=100, pick="nearest")
            closures = chunked.gate_closures([m if m >= 1 else -1 for m in matches])  # LCidx = match - 1 must exist
            closure_source = "generator (frame pairs within 0.3 m / 10 deg, SURVEY.md 8d)"
            det_info = None
            if e2e_traj is not None and e2e_closures is not None:
                # configs[2] / [3]: the closures of the end-to-end leg above -- the library's own detector with the reference's
                # scoring (a Hamming vocabulary tree, k 9 / L 6: src/bagOfWordsDetector.cpp:46-56; DBoW2's TF-IDF / L1 score
                # through the inverted file; GEOM_DI at di_levels 2, include/visualSLAM.h:120-127) over the ORB features
                # (cv::ORB's shape) of EVERY frame of the stitched stream, extracted by every rank on its own frames
                verdicts = e2e_traj[2]
                e2e_leg = legs.get("end_to_end", {})
                st_ = e2e_leg.get("rank0_stage_s", {})
                n_all = len(verdicts)
                det_info = {"frames": n_all, "ms_per_frame": st_.get("detector_own_share", 0.0) / max(1, n_all // world) * 1e3,
                            "feature_extraction_ms_per_frame": st_.get("features", 0.0) / max(1, share) * 1e3,
                            "scoring": "DBoW2 TF-IDF / L1 through an inverted file, GEOM_DI at di_levels 2; 16 frames per set of launches",
                            "features": "cv::ORB's shape (8 levels x 1.2, 500 features), 32 images per set of launches",
                            "vocabulary": legs.get("vocabulary"),
                            "detections": int(sum(v["status"] == 0 for v in verdicts)),
                            "accepted_closures": len(e2e_closures), "generator_closures": len(closures),
                            # an accepted closure is TRUE when the two frames' generator poses are within 2 m
                            "accepted_true": int(sum(np.linalg.norm(poses_all[q][1] - poses_all[m][1]) < 2.0
                                                     for q, m in e2e_closures.items()))}
                if e2e_closures:
                    closures = e2e_closures
                    closure_source = (f"svo_lc detector (vocabulary mode) on the ORB features of the stitched stream, extracted "
                                      f"by {world} rank(s) on their own frames (global frame ids)")
            ctxg = capi.Context(local_rank)
            pg = capi.PoseGraph(ctxg)
            ctxg.enable_kernel_timing(True)
            t0 = time.perf_counter()
            est, chi2 = chunked.global_solve(pg, traj, closures, iters=10)
            dt = time.perf_counter() - t0
            pg_ms, _ = ctxg.kernel_time(capi.K_POSEGRAPH)
            # the same solve once more on a fresh graph: the first one of a process pays for the lazy loading of its kernels
            pg2 = capi.PoseGraph(ctxg)
            chunked.global_solve(pg2, traj, closures, iters=10)
            pg_ms_total, _ = ctxg.kernel_time(capi.K_POSEGRAPH)
            pg2.close()
            result["posegraph"] = {
                "vertices": len(traj), "loop_closures": len(closures), "closure_source": closure_source,
                "detector": det_info, "gn_iterations": 10,
                "posegraph_ms_per_iter": pg_ms / 10.0,
                "posegraph_ms_per_iter_second_solve": (pg_ms_total - pg_ms) / 10.0,
                "solve_wall_ms_incl_graph_build": dt * 1e3,
                "chi2_first": float(chi2[0]), "chi2_last": float(chi2[-1]),
                "ate_rmse_vs_truth_before": ate_sh,
                "ate_rmse_vs_truth_after": chunked.ate_rmse(est[:, :3], t_truth),
            }
            pg.close()
            ctxg.close()
        except Exception as e:   # noqa: BLE001
            result["posegraph_error"] = f"{type(e).__name__}: {e}"

    trace("leg: cpu baseline")
    # ---- CPU baseline: the oracle on the node's own cores, a bounded sample of the same stream ----
    if rank == 0 and not args.no_cpu_baseline:
        try:   # an extra leg must not cost the run its line
            from oracle import orc  # the checker, timed as the CPU baseline ("port")

            native = orc.use_native_build()
            nf = min(max(2, args.cpu_frames), L)
            host = [(lefts[i].cpu().numpy(), rights[i].cpu().numpy()) for i in range(nf + 1)]

            def oracle_run(threads: int, frames: int):
                orc.set_num_threads(threads)
                o = orc.VO(W, H, C, grid_step=grid_step, anms_keep=n_kpts, keyframe_min_inliers=kf_min, seed=20261003)
                c0 = time.perf_counter()
                o.init(*host[0])
                out = []
                for i in range(1, frames + 1):
                    rc, R, t, *_ = o.track(*host[i])
                    if rc:
                        break
                    out.append((R.copy(), t.copy()))
                dt = time.perf_counter() - c0
                o.close()
                return (len(out) + 1) / dt, out

            cores = os.cpu_count() or 1
            # the thread count that is fastest on THIS node: a short sample at each candidate, the full sample at the best
            cands = sorted({t for t in (16, 32, 64, 128, cores) if t <= cores} or {cores})
            sweep = {}
            for tc in cands:
                sweep[tc] = oracle_run(tc, min(6, nf))[0]
            threads = max(sweep, key=sweep.get)
            multi, o_poses = oracle_run(threads, nf)
            single_thr, _ = oracle_run(1, max(3, nf // 4))
            g_poses = local[0][1:1 + len(o_poses)]   # chunk 0 of rank 0 started on the same frame with the same seed
            dts = [float(np.linalg.norm(tg - to)) for (Rg, tg), (Ro, to) in zip(g_poses, o_poses)]
            dRs = [rot_angle(Rg, Ro) for (Rg, tg), (Ro, to) in zip(g_poses, o_poses)]
            result["ate_rmse_vs_oracle"] = chunked.ate_rmse([t for _, t in g_poses], [t for _, t in o_poses])
            result["max_frame_delta_vs_oracle"] = {
                "translation_m": max(dts), "rotation_rad": max(dRs), "frames": len(dts),
                # arccos of a trace resolves 1e-8 rad at best: the entries themselves say whether the rotations are EQUAL
                "rotation_matrix_max_abs_diff": max(float(np.abs(Rg - Ro).max()) for (Rg, _), (Ro, _) in zip(g_poses, o_poses)),
                "bit_identical": all(np.array_equal(Rg, Ro) and np.array_equal(tg, to)
                                     for (Rg, tg), (Ro, to) in zip(g_poses, o_poses))}
            result["cpu_baseline"] = {
                "value": multi,
                "unit": "frames/s",
                "cores": threads,
                "host_cpu_count": cores,
                "kind": "port",
                "sample": f"chunk 0 of the same stream: stereo initialisation + {nf} frames, same stages, oracle C "
                          f"({'-O3 -march=native, built on this host' if native else '-O3 -march=x86-64-v3 (prebuilt)'}, "
                          f"OpenMP over keypoints in LK and ANMS and over the hypotheses' scoring passes in both RANSAC stages), "
                          f"{threads} threads = the fastest of {cands} on this node",
                "single_thread_value": single_thr,
                "thread_sweep_frames_per_s": {str(k): v for k, v in sweep.items()},
            }
        except Exception as e:   # noqa: BLE001
            result["cpu_baseline_error"] = f"{type(e).__name__}: {e}"

    if rank == 0:
        print(json.dumps(result), flush=True)
    if dist is not None:
        dist.barrier()
    if comm_state["thread"] is not None and comm_state["thread"].is_alive():
        # a helper thread is still inside RCCL on its own context: nothing of it was used; leave without unwinding it
        sys.stdout.flush()
        sys.stderr.flush()
        os._exit(0)
    if comm is not None:
        comm.close()
    if dist is not None:
        dist.destroy_process_group()
    if sh is not None:
        sh.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
