"""The multi-GPU path on CPU: chunk partitioning, and the all-gather of
chunk-boundary poses + rebasing under torch.distributed with the gloo backend, world size 2
and 3 (one process per rank, as one process per GPU on the node)."""
import os
import socket

import numpy as np
import pytest
from scipy.spatial.transform import Rotation as Rot

from ros_stereo_slam_amd import chunked


def test_chunk_bounds_cover_with_one_frame_overlap():
    for n, g in ((4541, 8), (200, 2), (10, 3), (5, 8), (2, 1)):
        b = chunked.chunk_bounds(n, g)
        assert b[0][0] == 0 and b[-1][1] == n - 1
        for (s0, e0), (s1, e1) in zip(b, b[1:]):
            assert e0 == s1 and e0 > s0
        sizes = [e - s for s, e in b]
        assert max(sizes) - min(sizes) <= 1
    assert chunked.chunk_bounds(4541, 8)[0] == (0, 568)
    with pytest.raises(ValueError):
        chunked.chunk_bounds(1, 2)


def _trajectory(n, seed=0):
    rng = np.random.default_rng(seed)
    poses = [(np.eye(3), np.zeros(3))]
    for _ in range(n - 1):
        dR = Rot.from_rotvec(rng.normal(0, 0.02, 3)).as_matrix()
        dt = np.array([0.0, 0.0, 0.9]) + rng.normal(0, 0.02, 3)
        poses.append(chunked.compose(*poses[-1], dR, dt))
    return poses


def test_prefix_and_rebase_reproduce_the_global_trajectory():
    gt = _trajectory(41)
    bounds = chunked.chunk_bounds(41, 4)
    local, boundaries = [], []
    for s, e in bounds:
        R0, t0 = gt[s]
        loc = [(R0.T @ R, R0.T @ (t - t0)) for R, t in gt[s:e + 1]]  # what a chunk's VO would output
        local.append(loc)
        boundaries.append(loc[-1])
    starts = chunked.prefix_transforms(boundaries)
    for (s, e), loc, st in zip(bounds, local, starts):
        for (R, t), (Rg, tg) in zip(chunked.rebase(loc, *st), gt[s:e + 1]):
            assert np.abs(R - Rg).max() < 1e-12 and np.abs(t - tg).max() < 1e-10


def test_pose7_and_ate():
    R = Rot.from_rotvec([0.3, -0.4, 2.9]).as_matrix()
    p = chunked.pose7(R, [1, 2, 3])
    assert np.abs(Rot.from_quat(p[3:]).as_matrix() - R).max() < 1e-14 and p[6] >= 0
    assert chunked.ate_rmse([[0, 0, 1], [0, 0, 2]], [[0, 0, 1], [0, 3, 2]]) == pytest.approx(np.sqrt(4.5))


def _worker(rank, world, port, n, q):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        gt = _trajectory(n)
        s, e = chunked.chunk_bounds(n, world)[rank]
        R0, t0 = gt[s]
        local = [(R0.T @ R, R0.T @ (t - t0)) for R, t in gt[s:e + 1]]
        mine, traj = chunked.stitch(dist, local)
        err_mine = max(np.abs(R - Rg).max() + np.abs(t - tg).max() for (R, t), (Rg, tg) in zip(mine, gt[s:e + 1]))
        err_traj = max(np.abs(R - Rg).max() + np.abs(t - tg).max() for (R, t), (Rg, tg) in zip(traj, gt))
        q.put((rank, len(traj), err_mine, err_traj))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_stitch_over_gloo(world):
    import torch.multiprocessing as mp

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    n = 25
    procs = [ctx.Process(target=_worker, args=(r, world, port, n, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert sorted(r[0] for r in res) == list(range(world))
    for rank, ntraj, e_mine, e_traj in res:
        assert ntraj == n                      # overlap frames are not duplicated
        assert e_mine < 1e-10 and e_traj < 1e-10


def _worker_multi(rank, world, port, n, m, q):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        gt = _trajectory(n)
        bounds = chunked.chunk_bounds(n, world * m)[rank * m:(rank + 1) * m]  # this rank's m chunks
        local = []
        for s, e in bounds:
            R0, t0 = gt[s]
            local.append([(R0.T @ R, R0.T @ (t - t0)) for R, t in gt[s:e + 1]])
        boundaries = chunked.all_gather_chunk_boundaries(dist, [loc[-1] for loc in local])
        starts = chunked.prefix_transforms(boundaries)
        err = 0.0
        for k, ((s, e), loc) in enumerate(zip(bounds, local)):
            for (R, t), (Rg, tg) in zip(chunked.rebase(loc, *starts[rank * m + k]), gt[s:e + 1]):
                err = max(err, np.abs(R - Rg).max() + np.abs(t - tg).max())
        q.put((rank, len(boundaries), err))
    finally:
        dist.destroy_process_group()


def test_several_chunks_per_rank_over_gloo():
    """svo_vo_run_chunks layout: every rank owns m chunks; one all-gather carries all m
    boundary poses of every rank and the global chunk order is rank-major."""
    import torch.multiprocessing as mp

    world, m, n = 2, 3, 37
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker_multi, args=(r, world, port, n, m, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, nb, err in res:
        assert nb == world * m and err < 1e-10


# ---- BASELINE configs[3] as one flow on CPU: shard -> all-gather -> rebase -> closures on global
# frame ids -> ONE global solve (fake VO = ground truth + drift; the oracle's pose graph solves) ----
def _drifting_loop(n, lap):
    """Ground truth: a circle of `lap` frames walked repeatedly; the fake VO's relative motions carry
    a constant yaw and forward bias, so its trajectory drifts away from the loop."""
    gt = []
    for i in range(n):
        a = 2 * np.pi * (i % lap) / lap
        gt.append((Rot.from_euler("y", a).as_matrix(), np.array([20 * (1 - np.cos(a)), 0.0, 20 * np.sin(a)])))
    bias_R = Rot.from_euler("y", 4e-4).as_matrix()
    rel = []
    for (Ra, ta), (Rb, tb) in zip(gt, gt[1:]):
        dR, dt = Ra.T @ Rb, Ra.T @ (tb - ta)
        rel.append((dR @ bias_R, dt * 1.004))
    return gt, rel


def _local_from_rel(rel, s, e):
    loc = [(np.eye(3), np.zeros(3))]
    for dR, dt in rel[s:e]:
        loc.append(chunked.compose(*loc[-1], dR, dt))
    return loc


def _configs3_flow(dist, rank, world, m, n, lap):
    from oracle import orc

    gt, rel = _drifting_loop(n, lap)
    share = (n - 1) // world
    s0 = rank * share
    bounds = chunked.chunk_bounds(share + 1, m)
    local = [_local_from_rel(rel, s0 + s, s0 + e) for s, e in bounds]
    traj = chunked.stitch_chunks(dist, local, device="cpu")
    matches = [i - lap if i >= lap else -1 for i in range(n)]
    closures = chunked.gate_closures(matches)
    pg = orc.PoseGraph()
    est, chi2 = chunked.global_solve(pg, traj, closures, iters=10)
    gt_t = np.array([t for _, t in gt])
    before = chunked.ate_rmse([t for _, t in traj], gt_t)
    after = chunked.ate_rmse(est[:, :3], gt_t)
    return len(traj), len(closures), before, after, float(chi2[0]), float(chi2[-1]), est


def _worker_configs3(rank, world, port, q):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        r = _configs3_flow(dist, rank, world, 3, 361, 120)
        q.put((rank,) + r[:6] + (float(np.abs(r[6]).sum()),))
    finally:
        dist.destroy_process_group()


def test_gate_closures_follows_the_reference_rule():
    m = [-1] * 300
    for q in (50, 150, 151, 200, 260):
        m[q] = q - 120 if q >= 120 else 0
    m[50] = 0           # only 50 frames back: refused (query - match must exceed 100)
    got = chunked.gate_closures(m)
    assert got == {150: 30, 260: 140}  # 151 and 200 fall into the 100-frame cooldown after 150


def test_configs3_flow_single_process_matches_two_ranks_over_gloo():
    import torch.multiprocessing as mp

    one = _configs3_flow(None, 0, 1, 6, 361, 120)
    assert one[0] == 361 and one[1] >= 2
    assert one[3] < 0.7 * one[2], f"global solve must pull the drift in: ATE {one[2]:.3f} -> {one[3]:.3f}"
    assert one[5] < 1e-3 * one[4]
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker_configs3, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=180) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, ntraj, ncl, before, after, c0, c1, checksum in res:
        assert ntraj == 361 and ncl == one[1]
        # the same chunks in the same order, whoever ran them: identical trajectory and solve
        assert before == pytest.approx(one[2], rel=1e-12) and after == pytest.approx(one[3], rel=1e-9)
        assert checksum == pytest.approx(float(np.abs(one[6]).sum()), rel=1e-9)


# ---- detector-driven closures at N > 1 (VERDICT r3 missing #2): every rank extracts the features of its own frames, rank 0
# keeps the database by global frame id -- over gloo with the ORACLE's extractor and detector (the GPU twins are compared
# with them in tests/test_gpu_orb.py / test_gpu_bow.py) ----
def _loop_images_small(n):
    from ros_stereo_slam_amd import synth

    size, K4 = (320, 120), (180.0, 180.0, 160.0, 60.0)
    poses = synth.loop_trajectory(n, half_x=6, half_z=10, radius=4, step=0.5)
    sc = synth.Scene(wall_x=14, z_min=-18, z_max=18)
    return [sc.render(R, t, K=K4, size=size)[0] for R, t in poses]      # the left views (stereo()[0]) without rendering the right ones


def _closures_of(feats):
    """train the vocabulary on every second frame, run the detector over all, gate as the reference does"""
    from oracle import orc
    from oracle.loop_detector import LoopDetector, Params

    voc = orc.Vocabulary.train([d for _, d in feats[::2]], k=9, L=4, seed=1)
    det = LoopDetector(Params(seed=5, n_features=200), voc=voc, di_levels=2)
    verdicts = [det.detect_features(xy, d) for xy, d in feats]
    matches = [v["match"] if v["status"] == 0 and v["match"] >= 1 else -1 for v in verdicts]
    return chunked.gate_closures(matches), [v["status"] for v in verdicts]


def _detector_worker(rank, world, port, n, q):
    import torch.distributed as dist

    from oracle import orc

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        imgs = _loop_images_small(n)
        share = (n - 1) // world
        lo, hi = rank * share, (rank + 1) * share + (1 if rank == world - 1 else 0)   # the overlap frame is the next rank's
        counts = [share + (1 if r == world - 1 else 0) for r in range(world)]
        nf = 200
        fn, fxy, fdesc = np.zeros(hi - lo, np.int32), np.zeros((hi - lo, nf, 2), np.float32), np.zeros((hi - lo, nf, 8), np.uint32)
        for i in range(lo, hi):
            xy, _, _, _, desc = orc.orb_extract(imgs[i], nf, 20)
            fn[i - lo] = len(xy)
            fxy[i - lo, :len(xy)], fdesc[i - lo, :len(xy)] = xy, desc
        parts = chunked.gather_frame_features(dist, fn, fxy, fdesc, counts=counts)
        if rank == 0:
            feats = [(pxy[i, :pn[i]], pd[i, :pn[i]]) for pn, pxy, pd in parts for i in range(len(pn))]
            q.put(("sharded", len(feats), _closures_of(feats)))
        else:
            assert parts is None
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_detector_closures_from_features_gathered_over_gloo():
    import torch.multiprocessing as mp

    from oracle import orc

    n, world = 141, 2
    imgs = _loop_images_small(n)
    single = [(xy, desc) for xy, _, _, _, desc in (orc.orb_extract(im, 200, 20) for im in imgs)]
    want_closures, want_status = _closures_of(single)
    assert want_closures, "the loop must close for the test to mean something"
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_detector_worker, args=(r, world, port, n, q)) for r in range(world)]
    for p in procs:
        p.start()
    tag, n_feats, (closures, status) = q.get(timeout=600)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert tag == "sharded" and n_feats == n
    assert closures == want_closures and status == want_status        # the two-rank flow gives the one-process verdicts


# ---- the detector SHARDED like the front-end: every rank fills its database with the frames before its
# share (entries that are not queries), queries its own frames after a short warm-up of the temporal window, rank 0 only
# gates the gathered verdicts.  The verdicts must be those of ONE detector over the whole stream. ----
def _sharded_detector_worker(rank, world, port, n, q, lc=None):
    import torch.distributed as dist

    from oracle import orc
    from oracle.loop_detector import LoopDetector, Params

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        imgs = _loop_images_small(n)
        shares = chunked.detect_shares(n, world)
        lo, hi = shares[rank]
        nf = 200
        fn, fxy, fdesc = np.zeros(hi - lo, np.int32), np.zeros((hi - lo, nf, 2), np.float32), np.zeros((hi - lo, nf, 8), np.uint32)
        for i in range(lo, hi):
            xy, _, _, _, desc = orc.orb_extract(imgs[i], nf, 20)
            fn[i - lo] = len(xy)
            fxy[i - lo, :len(xy)], fdesc[i - lo, :len(xy)] = xy, desc
        an, axy, adesc = chunked.all_gather_frame_features(dist, fn, fxy, fdesc, counts=[e - s for s, e in shares])
        feats = [(axy[i, :an[i]], adesc[i, :an[i]]) for i in range(n)]
        voc = orc.Vocabulary.train([d for _, d in feats[::2]], k=9, L=4, seed=1)      # every rank: the same vocabulary
        det = LoopDetector(Params(seed=5, n_features=200, **(lc or {})), voc=voc, di_levels=2)
        queue = []

        def fill(a, b):
            for i in range(a, b):
                det.fill(*feats[i])

        def submit(a, b):
            queue.extend(range(a, b))

        def collect():
            i = queue.pop(0)
            return det.detect_features(*feats[i])

        mine = chunked.sharded_detect(fill, submit, collect, lo, hi, params=det.p if lc else None)
        assert len(mine) == hi - lo and all(v["query"] == lo + k for k, v in enumerate(mine))
        allv = chunked.gather_verdicts(dist, mine, shares)
        if rank == 0:
            matches = [v["match"] if v["status"] == 0 and v["match"] >= 1 else -1 for v in allv]
            q.put(("sharded detector", chunked.gate_closures(matches), [v["status"] for v in allv], [v["match"] for v in allv]))
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_detector_sharded_over_gloo_gives_the_one_detector_verdicts(world):
    import torch.multiprocessing as mp

    from oracle import orc
    from oracle.loop_detector import LoopDetector, Params

    n = 141
    imgs = _loop_images_small(n)
    feats = [(xy, desc) for xy, _, _, _, desc in (orc.orb_extract(im, 200, 20) for im in imgs)]
    voc = orc.Vocabulary.train([d for _, d in feats[::2]], k=9, L=4, seed=1)
    det = LoopDetector(Params(seed=5, n_features=200), voc=voc, di_levels=2)
    want = [det.detect_features(xy, d) for xy, d in feats]
    want_closures = chunked.gate_closures([v["match"] if v["status"] == 0 and v["match"] >= 1 else -1 for v in want])
    assert want_closures
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_sharded_detector_worker, args=(r, world, port, n, q)) for r in range(world)]
    for p in procs:
        p.start()
    tag, closures, status, match = q.get(timeout=900)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert tag == "sharded detector"
    assert status == [v["status"] for v in want] and match == [v["match"] for v in want]
    assert closures == want_closures


@pytest.mark.parametrize("k,world", [(3, 2), (3, 3), (9, 2), (9, 3)])
def test_detector_sharded_over_gloo_at_larger_k(k, world):
    """The same flow at k 3 and k 9, sharded_detect told the detector's parameters (alpha 0.01 lets nearly every frame reach
    the window, which is then longer than k where the later ranks' shares begin: the case the fixed warm-up of 8 frames got
    wrong at k 9)."""
    import torch.multiprocessing as mp

    from oracle import orc
    from oracle.loop_detector import LoopDetector, Params

    n, lc = 141, dict(alpha=float(np.float32(0.01)), k=k)
    imgs = _loop_images_small(n)
    feats = [(xy, desc) for xy, _, _, _, desc in (orc.orb_extract(im, 200, 20) for im in imgs)]
    voc = orc.Vocabulary.train([d for _, d in feats[::2]], k=9, L=4, seed=1)
    det = LoopDetector(Params(seed=5, n_features=200, **lc), voc=voc, di_levels=2)
    want = [det.detect_features(xy, d) for xy, d in feats]
    assert all(want[first]["status"] in (0, 7) for first, _ in chunked.detect_shares(n, world)[1:])   # the window is past k there
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_sharded_detector_worker, args=(r, world, port, n, q, lc)) for r in range(world)]
    for p in procs:
        p.start()
    tag, closures, status, match = q.get(timeout=900)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert tag == "sharded detector"
    assert status == [v["status"] for v in want] and match == [v["match"] for v in want]


def test_poses7_is_pose7_element_by_element():
    """chunked.poses7 (one pass over arrays) against chunked.pose7 (one pose at a time): the same bits, also for rotations
    by nearly pi about every axis (the three branches of the quaternion extraction with a negative trace)."""
    from scipy.spatial.transform import Rotation as Rot

    from ros_stereo_slam_amd import chunked

    rng = np.random.default_rng(1)
    Rs = Rot.random(600, random_state=3).as_matrix()
    axes = rng.normal(size=(90, 3))
    axes /= np.linalg.norm(axes, axis=1)[:, None]
    Rs[:90] = Rot.from_rotvec(axes * (np.pi * (1 - 1e-6 * rng.random((90, 1))))).as_matrix()
    Rs[90:93] = [np.diag([1.0, -1.0, -1.0]), np.diag([-1.0, 1.0, -1.0]), np.diag([-1.0, -1.0, 1.0])]
    ts = rng.normal(size=(600, 3))
    traj = [(Rs[i], ts[i]) for i in range(600)]
    one = np.array([chunked.pose7(*p) for p in traj])
    assert np.array_equal(one, chunked.poses7(traj))
    assert chunked.poses7([]).shape == (0, 7)
