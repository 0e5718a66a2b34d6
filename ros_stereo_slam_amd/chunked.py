"""Chunk-sharded stereo VO across GPUs (BASELINE.json configs[3]).

The front-end is sequential in time (frame n needs frame n-1's surviving points and pose,
``src/VisualSLAM.cpp:54-169``), so a sequence shards across GPUs only in time: rank g owns
the contiguous frames ``[s_g, s_{g+1}]`` -- INCLUDING the first frame of the next chunk, so
that its last pose is the boundary transform ``T(s_g -> s_{g+1})`` -- re-initialises at
``s_g`` (stereo keyframe, identity pose) and runs the ordinary front-end.  The path's one
exchange step is an all-gather of the boundary transforms (12 doubles per rank, over RCCL
when the process group is ``nccl``); every rank then composes the prefix
``T(0 -> s_g) = prod_{h<g} T(s_h -> s_{h+1})`` and rebases its local poses.  The rebased
trajectories feed one global pose graph (``PoseGraph``) whose loop closures use global
frame ids.

Results differ from the single-GPU run by construction (extra keyframes at chunk starts);
the stated tolerance is on the trajectory (ATE), not per frame.
"""
from __future__ import annotations

import numpy as np


def chunk_bounds(n_frames: int, n_chunks: int) -> list[tuple[int, int]]:
    """Inclusive frame ranges ``[(s_g, e_g)]`` with ``e_g = s_{g+1}`` (one frame of overlap).

    Frames are split as evenly as possible; the last chunk ends at ``n_frames - 1``."""
    if n_chunks < 1 or n_frames < 2:
        raise ValueError("need at least one chunk and two frames")
    n_chunks = min(n_chunks, n_frames - 1)
    steps = n_frames - 1  # number of frame-to-frame transitions
    base, extra = divmod(steps, n_chunks)
    bounds, s = [], 0
    for g in range(n_chunks):
        e = s + base + (1 if g < extra else 0)
        bounds.append((s, e))
        s = e
    return bounds


def compose(Ra, ta, Rb, tb):
    """Pose composition ``T_a * T_b`` for camera-in-world poses (X_w = R X_c + t)."""
    return Ra @ Rb, Ra @ tb + ta


def rebase(local_poses, R0, t0):
    """Re-express chunk-local poses (relative to the chunk's first frame) in the global frame."""
    return [compose(R0, t0, R, t) for (R, t) in local_poses]


def prefix_transforms(boundaries):
    """``boundaries[g] = (R, t)`` of chunk g's last frame in chunk g's own frame.
    Returns the global pose of each chunk's FIRST frame: identity, B0, B0*B1, ..."""
    out = [(np.eye(3), np.zeros(3))]
    for (R, t) in boundaries[:-1]:
        out.append(compose(*out[-1], R, t))
    return out


def _all_gather_flat(dist, mine, group=None):
    """One ``all_gather_into_tensor`` of equally sized 1-D tensors -> (world, numel) (the flat in / flat out form is the one
    every backend -- nccl == RCCL, gloo -- accepts)."""
    import torch

    mine = mine.reshape(-1).contiguous()
    got = torch.empty(dist.get_world_size() * mine.numel(), dtype=mine.dtype, device=mine.device)
    dist.all_gather_into_tensor(got, mine, group=group)
    return got.reshape(dist.get_world_size(), mine.numel())


def all_gather_boundaries(dist, R, t, device=None, n_poses=None):
    """The path's one collective: every rank contributes its chunk-boundary pose (12 doubles)
    and receives all of them.  ``dist`` is ``torch.distributed`` (backend nccl == RCCL on the
    GPU node, gloo in the CPU tests).  ``n_poses``: this rank's pose count rides along as a 13th
    double (chunks may differ by a frame); the result is then (boundaries, counts)."""
    import torch

    dev = device if device is not None else ("cuda" if dist.get_backend() == "nccl" else "cpu")
    row = np.r_[np.asarray(R, np.float64).ravel(), np.asarray(t, np.float64).ravel(),
                [] if n_poses is None else [float(n_poses)]]
    a = _all_gather_flat(dist, torch.tensor(row, dtype=torch.float64, device=dev)).cpu().numpy()
    res = [(r[:9].reshape(3, 3).copy(), r[9:12].copy()) for r in a]
    if n_poses is None:
        return res
    return res, [int(r[12]) for r in a]


def all_gather_chunk_boundaries(dist, pairs, device=None, comm=None, group=None):
    """As :func:`all_gather_boundaries` when every rank runs several chunks side by side
    (``svo_vo_run_chunks``): ``pairs`` = this rank's chunk-boundary poses in chunk order, the
    same number on every rank.  Still ONE all-gather (12 doubles per chunk); returns the
    boundaries of all chunks in global chunk order (rank-major).

    ``comm``: a ``capi.ShardComm`` -- the collective then runs behind the C ABI
    (``svo_shard_allgather_boundaries``: ncclAllGather on the context's stream), which is what a C++ host
    calls; ``dist`` is not touched."""
    if comm is not None:
        return comm.allgather_boundaries(pairs)
    import torch

    dev = device if device is not None else ("cuda" if dist.get_backend() == "nccl" else "cpu")
    return array_to_poses(_all_gather_flat(dist, torch.from_numpy(poses_to_array(pairs)).to(dev), group=group).cpu().numpy())


def poses_to_array(poses) -> np.ndarray:
    """[(R, t)] -> (n, 12) float64 rows [R row-major | t]."""
    if isinstance(poses, np.ndarray):
        return np.ascontiguousarray(poses, np.float64).reshape(-1, 12)
    out = np.empty((len(poses), 12))
    for i, (R, t) in enumerate(poses):
        out[i, :9] = np.asarray(R, np.float64).ravel()
        out[i, 9:] = np.asarray(t, np.float64).ravel()
    return out


def array_to_poses(a):
    return [(r[:9].reshape(3, 3).copy(), r[9:].copy()) for r in np.asarray(a).reshape(-1, 12)]


def gather_trajectories(dist, poses, device=None, counts=None, as_array=False):
    """All ranks receive every rank's (rebased) poses -- ONE tensor collective (``all_gather_into_tensor`` of
    max(counts) x 12 doubles per rank).  ``counts``: every rank's pose count, which the callers know without a
    second exchange (equal shares: the bench; unequal chunks: it rode along with the boundary all-gather, see
    :func:`all_gather_boundaries`); None = every rank holds ``len(poses)``.  Returns one pose list per rank, or
    with ``as_array`` one (count, 12) array per rank (no per-pose Python objects)."""
    import torch

    dev = device if device is not None else ("cuda" if dist.get_backend() == "nccl" else "cpu")
    world = dist.get_world_size()
    mine_a = poses_to_array(poses)
    if counts is None:   # ranks may hold different numbers of poses: a small exchange of the counts first
        cnt = _all_gather_flat(dist, torch.tensor([len(mine_a)], dtype=torch.int64, device=dev))
        counts = [int(c) for c in cnt.cpu().numpy().ravel()]
    m = max(counts)
    host = np.zeros((m, 12))
    host[:len(mine_a)] = mine_a
    a = _all_gather_flat(dist, torch.from_numpy(host).to(dev)).cpu().numpy().reshape(world, m, 12)
    parts = [a[r, :c].copy() for r, c in enumerate(counts)]
    return parts if as_array else [array_to_poses(p) for p in parts]


def gather_frame_features(dist, n, xy, desc, counts=None, dst: int = 0, device=None):
    """The loop detector's input in a chunk-sharded run: every rank holds the ORB features of ITS frames -- ``n`` [F]
    feature counts, ``xy`` [F, nf, 2] float32, ``desc`` [F, nf, 8] uint32 (500 x 40 B per frame) -- and rank ``dst``,
    which keeps the database, receives them in rank order (global frame order).  ``counts``: frames per rank.  One
    gather per array; returns [(n, xy, desc)] per rank on ``dst``, None elsewhere."""
    import torch

    world, rank = dist.get_world_size(), dist.get_rank()
    # host tensors over gloo; over nccl (= RCCL) the bytes travel through device tensors and come back with .cpu()
    dev = device if device is not None else ("cuda" if dist.get_backend() == "nccl" else "cpu")
    n = np.ascontiguousarray(n, np.int32)
    xy = np.ascontiguousarray(xy, np.float32)
    desc = np.ascontiguousarray(desc, np.uint32)
    if counts is None:
        counts = [len(n)] * world
    m, nf = max(counts), xy.shape[1]

    def pad(a, shape, dtype):
        out = np.zeros(shape, dtype)
        out[:len(a)] = a
        return torch.from_numpy(out.view(np.uint8).reshape(-1)).to(dev)

    out = []
    for a, shape, dtype in ((n, (m,), np.int32), (xy, (m, nf, 2), np.float32), (desc, (m, nf, 8), np.uint32)):
        mine = pad(a, shape, dtype)
        got = [torch.empty_like(mine) for _ in range(world)] if rank == dst else None
        dist.gather(mine, got, dst=dst)
        out.append(None if got is None else [g.cpu().numpy().view(dtype).reshape(shape) for g in got])
    if rank != dst:
        return None
    return [(out[0][r][:counts[r]], out[1][r][:counts[r]], out[2][r][:counts[r]]) for r in range(world)]


def stitch(dist, local_poses, device=None):
    """Rank-local poses (relative to the chunk's first frame, one per frame of the chunk
    including the overlap frame) -> the rank's poses in the global frame, plus the global
    trajectory without the duplicated overlap frames (identical on every rank)."""
    rank = dist.get_rank()
    boundaries, counts = all_gather_boundaries(dist, *local_poses[-1], device=device, n_poses=len(local_poses))
    starts = prefix_transforms(boundaries)
    mine = rebase(local_poses, *starts[rank])
    chunks = gather_trajectories(dist, mine, device=device, counts=counts)
    traj = list(chunks[0])
    for ch in chunks[1:]:
        traj.extend(ch[1:])  # the first frame of a chunk is the last frame of the previous one
    return mine, traj


def run_chunk(vo, frames):
    """Runs the front-end over one chunk.  ``frames``: iterable of (left, right) images (host
    arrays or device tensors); the first one seeds the chunk (identity pose).  Returns the list
    of chunk-local (R, t), one per frame, and per-frame stats."""
    it = iter(frames)
    left, right = next(it)
    vo.init(left, right)
    poses = [(np.eye(3), np.zeros(3))]
    stats = []
    for left, right in it:
        rc, R, t, ninl, kf, ntrk = vo.track(left, right)
        if rc:
            raise RuntimeError(f"tracking lost in chunk at local frame {len(poses)}")
        poses.append((R.copy(), t.copy()))
        stats.append((ninl, kf, ntrk))
    return poses, stats


def pose7(R, t):
    """(R, t) -> tx ty tz qx qy qz qw (the pose-graph layout)."""
    R = np.asarray(R, np.float64)
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr > 0:
        s = np.sqrt(tr + 1.0) * 2
        q = [(R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s, 0.25 * s]
    elif R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
        s = np.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2]) * 2
        q = [0.25 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s, (R[2, 1] - R[1, 2]) / s]
    elif R[1, 1] > R[2, 2]:
        s = np.sqrt(1.0 + R[1, 1] - R[0, 0] - R[2, 2]) * 2
        q = [(R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + R[2, 1]) / s, (R[0, 2] - R[2, 0]) / s]
    else:
        s = np.sqrt(1.0 + R[2, 2] - R[0, 0] - R[1, 1]) * 2
        q = [(R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s, (R[1, 0] - R[0, 1]) / s]
    q = np.array(q)
    if q[3] < 0:
        q = -q
    return np.r_[np.asarray(t, np.float64), q / np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])]


def poses7(traj):
    """[(R, t)] -> [n, 7]: :func:`pose7` of every pose in one pass over arrays (the same operations element by element; the
    per-pose form costs 6 ... 14 us of interpreter time, which at thousands of frames is more than the solve they feed)."""
    n = len(traj)
    if n == 0:
        return np.zeros((0, 7))
    R = np.array([np.asarray(p[0], np.float64) for p in traj]).reshape(n, 3, 3)
    t = np.array([np.asarray(p[1], np.float64).reshape(3) for p in traj])
    r00, r11, r22 = R[:, 0, 0], R[:, 1, 1], R[:, 2, 2]
    tr = r00 + r11 + r22
    c0 = tr > 0
    c1 = ~c0 & (r00 > r11) & (r00 > r22)
    c2 = ~c0 & ~c1 & (r11 > r22)
    c3 = ~(c0 | c1 | c2)
    with np.errstate(invalid="ignore", divide="ignore"):
        s0 = np.sqrt(tr + 1.0) * 2
        s1 = np.sqrt(1.0 + r00 - r11 - r22) * 2
        s2 = np.sqrt(1.0 + r11 - r00 - r22) * 2
        s3 = np.sqrt(1.0 + r22 - r00 - r11) * 2
        q = np.zeros((n, 4))
        for c, comp in ((c0, ((R[:, 2, 1] - R[:, 1, 2]) / s0, (R[:, 0, 2] - R[:, 2, 0]) / s0, (R[:, 1, 0] - R[:, 0, 1]) / s0, 0.25 * s0)),
                        (c1, (0.25 * s1, (R[:, 0, 1] + R[:, 1, 0]) / s1, (R[:, 0, 2] + R[:, 2, 0]) / s1, (R[:, 2, 1] - R[:, 1, 2]) / s1)),
                        (c2, ((R[:, 0, 1] + R[:, 1, 0]) / s2, 0.25 * s2, (R[:, 1, 2] + R[:, 2, 1]) / s2, (R[:, 0, 2] - R[:, 2, 0]) / s2)),
                        (c3, ((R[:, 0, 2] + R[:, 2, 0]) / s3, (R[:, 1, 2] + R[:, 2, 1]) / s3, 0.25 * s3, (R[:, 1, 0] - R[:, 0, 1]) / s3))):
            for k in range(4):
                q[c, k] = comp[k][c]
    q[q[:, 3] < 0] *= -1
    q /= np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])[:, None]
    return np.concatenate([t, q], axis=1)


def ate_rmse(est_t, gt_t):
    """Absolute trajectory error (RMSE of the translation difference, no alignment: both
    trajectories start at the identity pose of frame 0)."""
    d = np.asarray(est_t, np.float64) - np.asarray(gt_t, np.float64)
    return float(np.sqrt(np.mean(np.sum(d * d, axis=1))))


# ---- BASELINE configs[3] as one callable: shard -> all-gather -> rebase -> closures on global ids ->
# ONE global solve (src/VisualSLAM.cpp:76-86, include/poseGraph.h:113-138) -------------
class ShardedVO:
    """One rank's share of a chunk-sharded stream: ``n_chunks`` contiguous chunks of the rank's
    frames run side by side on this GPU (``svo_vo_run_chunks``), ``chunks_per_context`` of them per
    context in lock step.  Every chunk re-initialises at its first frame (stereo keyframe, identity
    pose) inside the same call."""

    def __init__(self, capi, device: int, w: int, h: int, c: int, n_chunks: int, chunks_per_context: int = 16,
                 first_chunk_id: int = 0, seed: int = 0, **vo_kwargs):
        self.capi = capi
        self.n_chunks = n_chunks
        g = max(1, min(16, chunks_per_context))
        self.ctxs = [capi.Context(device) for _ in range((n_chunks + g - 1) // g)]
        self.vos = [capi.VisualOdometry(self.ctxs[m // g], w, h, c, seed=seed + first_chunk_id + m, **vo_kwargs)
                    for m in range(n_chunks)]

    def run(self, lefts, rights, pipeline: bool = False):
        """``lefts`` / ``rights``: this rank's frames INCLUDING the first frame of the next rank's
        share (one frame of overlap).  Returns (local, stats): ``local[m]`` = chunk m's poses relative
        to its own first frame, one per frame of the chunk incl. its overlap frame; ``stats[m]`` =
        (inliers, tracked, keyframe) arrays.  Raises when a chunk loses tracking."""
        bounds = chunk_bounds(len(lefts), self.n_chunks)
        jobs = [(v, lefts[s:e + 1], rights[s:e + 1]) for v, (s, e) in zip(self.vos, bounds)]
        res = self.capi.run_chunks(jobs, pipeline=pipeline, init=True)
        local, stats = [], []
        for (s, e), (rc, done, R, t, inl, trk, kf) in zip(bounds, res):
            if rc or done != e - s:
                raise RuntimeError(f"chunk [{s}, {e}]: tracking lost after {done} frames (rc {rc})")
            local.append([(np.eye(3), np.zeros(3))] + [(R[i].copy(), t[i].copy()) for i in range(done)])
            stats.append((inl, trk, kf))
        return local, stats

    def sync(self):
        for c in self.ctxs:
            c.sync()

    def close(self):
        for v in self.vos:
            v.close()
        for c in self.ctxs:
            c.close()


def join_chunks(local, starts):
    """Chunk-local pose lists + the global pose of every chunk's first frame -> one pose list without
    the duplicated overlap frames."""
    traj = []
    for k, (loc, st) in enumerate(zip(local, starts)):
        glob = rebase(loc, *st)
        traj.extend(glob if k == 0 else glob[1:])
    return traj


def stitch_chunks(dist, local, device=None):
    """The exchange step for a rank that ran several chunks: ONE all-gather of the chunk-boundary
    poses (12 doubles per chunk), prefix composition, rebase, then the gather of the rebased
    trajectories.  ``dist`` None = single process.  Returns the global trajectory [(R, t)] (identical
    on every rank)."""
    pairs = [loc[-1] for loc in local]
    if dist is None:
        return join_chunks(local, prefix_transforms(pairs))
    rank, m = dist.get_rank(), len(local)
    boundaries = all_gather_chunk_boundaries(dist, pairs, device=device)
    starts = prefix_transforms(boundaries)
    mine = join_chunks(local, starts[rank * m:(rank + 1) * m])
    # join_chunks rebases chunk 0 of this rank with starts[rank*m], so `mine` is already global; ranks may hold
    # different numbers of frames: the counts take one small all-gather of their own here
    import torch

    dev = device if device is not None else ("cuda" if dist.get_backend() == "nccl" else "cpu")
    cnt = _all_gather_flat(dist, torch.tensor([len(mine)], dtype=torch.int64, device=dev))
    parts = gather_trajectories(dist, mine, device=device, counts=[int(c) for c in cnt.cpu().numpy().ravel()])
    traj = list(parts[0])
    for p in parts[1:]:
        traj.extend(p[1:])  # a rank's first frame is the previous rank's last
    return traj


def global_solve(pg, traj, closures, iters: int = 10):
    """The single global pose-graph solve of the sharded mode: vertices in frame order with the
    reference's staging (a closure detected at frame q adds the identity edge from vertex q-1 to
    ``LCidx = match - 1`` BEFORE vertex q is added, src/optimizationStuff.cpp:3-15,58-63), then one
    ``globalOptimize`` (include/poseGraph.h:128-138).  ``closures``: {query frame: matched frame} on
    GLOBAL frame ids.  Returns (estimates [n, 7], chi2 [iters + 1])."""
    n = len(traj)
    lc = np.full(n, -1, np.int32)
    for q, m in (closures or {}).items():
        if 1 <= q < n and m >= 0:
            lc[q] = max(m - 1, 0)
    if n > 1:
        if hasattr(pg, "augment_nodes"):     # svo_pg_augment_nodes: the whole chain in one call
            pg.augment_nodes(poses7(traj[1:]), lc[1:])
        else:
            p7 = poses7(traj[1:])
            for q in range(1, n):
                if lc[q] >= 0:
                    pg.add_loop_closure(int(lc[q]))
                pg.augment_node(p7[q - 1])
    chi2 = pg.optimize(iters)
    return pg.estimates(), chi2


def gate_closures(matches, min_gap: int = 100, cooldown: int = 100):
    """The reference's acceptance rule applied to a per-frame match list (-1 = none): accept iff
    ``query - match > min_gap`` and the cooldown has run out, then hold off for ``cooldown`` frames
    (src/optimizationStuff.cpp:58-63, src/VisualSLAM.cpp:148-150).  -> {query: match}."""
    out, cd = {}, 0
    for q, m in enumerate(matches):
        if m >= 0 and q - m > min_gap and cd == 0:
            out[q] = m
            cd = cooldown
        if cd:
            cd -= 1
    return out


# ---- the loop detector sharded like the front-end (the detector off rank 0's serial path) ----------------
DETECT_WARMUP = 8   # frames a rank queries BEFORE its share (verdicts discarded): they bring the temporal window into the
                    # state the sequential run has there -- the window forgets everything older than
                    # max_distance_between_queries (2) frames and is only ever compared with k (1); other settings:
                    # detect_warmup and sharded_detect's ``params``


def detect_shares(n_frames: int, world: int):
    """[(first, end)] of every rank's share of the QUERIES: frames first .. end - 1, contiguous, in rank order"""
    base, extra = divmod(n_frames, world)
    out, s = [], 0
    for r in range(world):
        e = s + base + (1 if r < extra else 0)
        out.append((s, e))
        s = e
    return out


def detect_warmup(k: int, max_distance_between_queries: int) -> int:
    """The fewest warm-up frames after which a detector that starts with an EMPTY temporal window judges as one that has seen
    the whole stream: ``k * max_distance_between_queries``.

    The window's update rule (updateTemporalWindow, include/TemplatedLoopDetector.h:966-1003) makes ``nentries`` the length of
    the current CHAIN of updates: an update at query q continues the chain iff the previous update was at most
    max_distance_between_queries (D) queries back and its island fits, else the chain restarts at 1.  Frames that stop before the
    islands (low scores, no groups ...) make no update.  A detector that starts empty at frame s holds the same chain cut to the
    updates at frames >= s, and a verdict reads the length only as ``nentries > k``.  So a frame f is judged alike iff the cut
    chain still has more than k links whenever the whole one has.  Links are at most D frames apart, so going back from the
    link at f the j-th earlier one lies at f - j D or later: the frames s .. f hold at least floor((f - s) / D) + 1 links of a
    chain that reaches back past s (and the whole chain otherwise).  That is more than k for every f >= first as soon as
    first - s >= k D.  With D <= 0 every update restarts the chain and with k <= 0 its length is never short: no warm-up at all.
    The bound is met with equality by a stream whose every D-th frame alone reaches the islands."""
    return max(int(k), 0) * max(int(max_distance_between_queries), 0)


def sharded_detect(fill, submit, collect, first: int, end: int, warmup: int = DETECT_WARMUP, collect_many=None, params=None):
    """One rank's part of the detection over a stream whose features every rank holds: the frames before the share enter
    the database WITHOUT being queries (``fill(a, b)``: frames a .. b - 1; svo_lc_fill_features_batch), then the share --
    preceded by ``warmup`` frames whose verdicts are discarded -- is queued (``submit(a, b)``) and collected
    (``collect()`` -> dict(status, query, match); ``collect_many(k)`` -> a list of k of them, if given).  Returns the verdicts of frames first .. end - 1, which are those of ONE
    detector run over the whole stream: a query's candidates, scores and normalisation score depend on the database alone,
    the temporal window on the last few queries alone.

    How few "the last few" are depends on the detector: ``params`` -- a mapping or an object with ``k`` and
    ``max_distance_between_queries``, e.g. the detector's svo_lc_params -- lengthens the warm-up to :func:`detect_warmup` of
    them where ``warmup`` is shorter.  Without ``params`` the warm-up is ``warmup`` as given, which is enough for the
    reference's k 1 / max_distance_between_queries 2 (2 frames) and for every setting with k * max_distance_between_queries
    <= 8."""
    if params is not None:
        get = params.__getitem__ if hasattr(params, "keys") else lambda name: getattr(params, name)
        warmup = max(warmup, detect_warmup(get("k"), get("max_distance_between_queries")))
    start = max(0, first - warmup)
    fill(0, start)
    # queued a piece ahead of the collection: host arrays go through the detector's small ring of pinned slots, so a submit
    # of everything would return only when the device has taken nearly all of it -- and the geometric checks, which run
    # from collect(), would start after the whole scoring pass instead of beside it
    piece, verdicts, queued = 64, [], start
    while len(verdicts) < end - start:
        while queued < end and queued - (start + len(verdicts)) < 2 * piece:
            b = min(end, queued + piece)
            submit(queued, b)
            queued = b
        k = min(piece, queued - (start + len(verdicts)))
        if collect_many is not None:   # ``collect_many(k)`` -> k verdicts in one call (svo_lc_collect_batch)
            verdicts.extend(collect_many(k))
        else:
            for _ in range(k):
                verdicts.append(collect())
    return verdicts[first - start:]


def gather_verdicts(dist, verdicts, shares, dst: int = 0):
    """(status, match) of every rank's share -> rank ``dst`` receives the whole stream's verdicts in frame order (one small
    gather of int32 pairs); None elsewhere."""
    import torch

    world, rank = dist.get_world_size(), dist.get_rank()
    m = max(e - s for s, e in shares)
    mine = np.full((m, 2), -1, np.int32)
    for i, v in enumerate(verdicts):
        mine[i] = (v["status"], v["match"])
    t = torch.from_numpy(mine.reshape(-1))
    got = [torch.empty_like(t) for _ in range(world)] if rank == dst else None
    dist.gather(t, got, dst=dst)
    if rank != dst:
        return None
    out = []
    for r, (s, e) in enumerate(shares):
        a = got[r].numpy().reshape(m, 2)
        out.extend(dict(status=int(a[i, 0]), match=int(a[i, 1]), query=s + i) for i in range(e - s))
    return out


def all_gather_frame_features(dist, n, xy, desc, counts, device=None, comm=None):
    """Every rank receives every rank's frame features (n [F], xy [F, nf, 2], desc [F, nf, 8]) in frame order: what the
    sharded detector needs (a query's geometric check reads the matched OLD frame's keys and descriptors, which may
    belong to any earlier rank).  ONE all-gather of a packed byte buffer per rank (n | xy | desc, padded to the largest
    share): through ``comm`` (a ``capi.ShardComm``: ncclAllGather behind the C ABI, ``svo_shard_allgather_bytes``) when given,
    else ``all_gather_into_tensor`` on ``dist``.  -> (n, xy, desc) of the whole stream."""
    world = comm.nranks if comm is not None else dist.get_world_size()
    m, nf = max(counts), xy.shape[1]
    parts = ((np.ascontiguousarray(n, np.int32), (m,), np.int32), (np.ascontiguousarray(xy, np.float32), (m, nf, 2), np.float32),
             (np.ascontiguousarray(desc, np.uint32), (m, nf, 8), np.uint32))
    sizes = [int(np.prod(shape)) * np.dtype(dt).itemsize for _, shape, dt in parts]
    host = np.zeros(sum(sizes), np.uint8)
    off = 0
    for (a, shape, dt), sz in zip(parts, sizes):
        view = host[off:off + sz].view(dt).reshape(shape)
        view[:len(a)] = a
        off += sz
    if comm is not None:
        got = comm.allgather_bytes(host)
    else:
        import torch

        dev = device if device is not None else ("cuda" if dist.get_backend() == "nccl" else "cpu")
        got = _all_gather_flat(dist, torch.from_numpy(host).to(dev)).cpu().numpy()
    out, off = [], 0
    for (a, shape, dt), sz in zip(parts, sizes):
        out.append(np.concatenate([got[r, off:off + sz].view(dt).reshape(shape)[:counts[r]] for r in range(world)]))
        off += sz
    return tuple(out)
