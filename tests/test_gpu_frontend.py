"""GPU parity of the whole front-end (svo_vo) against the oracle's frame loop on identical
synthetic frames.  Tolerances: while the inlier sets agree, per-frame pose
translation <= 1e-3 m and rotation <= 1e-4 rad; frames whose sets differ are reported."""
import numpy as np
import pytest

from ros_stereo_slam_amd import capi, synth

pytestmark = pytest.mark.gpu


def _frames(n, size=(1241, 376)):
    sc = synth.Scene()
    poses = synth.corridor_trajectory(n)
    return poses, [sc.stereo(R, t, size=size)[:2] for R, t in poses]


def _rot_angle(Ra, Rb):
    c = (np.trace(Ra.T @ Rb) - 1) / 2
    return float(np.arccos(np.clip(c, -1, 1)))


def _loop_frames(n):
    """The benchmark's stream (synth.BENCH_LOOP), rendered on the GPU: host copies for the oracle."""
    import torch

    poses = synth.loop_trajectory(n, **synth.BENCH_LOOP)
    lefts, rights = synth.stereo_torch(synth.bench_scene(), poses, device="cuda", batch=8)
    torch.cuda.synchronize()
    R0, t0 = poses[0]
    rel = [(R0.T @ R, R0.T @ (t - t0)) for R, t in poses]
    return rel, [(l.cpu().numpy(), r.cpu().numpy()) for l, r in zip(lefts, rights)]


@pytest.mark.parametrize("grid_step,anms_keep,kf_min,nframes", [(10, 4096, 2000, 201), (7, 8192, 4000, 41)])
def test_frontend_matches_oracle_on_the_benchmark_stream(ctx, orc, grid_step, anms_keep, kf_min, nframes):
    """The benchmarked shapes -- 4096 keypoints (the metric) over 200 frames (configs[0]'s length), 8192
    (configs[4]) over 40 -- frame by frame against the oracle's frame loop.  GPU and oracle share one software
    implementation of every transcendental function on the path (include/svo_math.h), so there is NO relaxed
    regime: every frame's tracked count, PnP inlier count, keyframe decision AND POSE must be EQUAL, bit for bit
    (SURVEY.md 8d allows 1e-3 m / 1e-4 rad)."""
    poses, frames = _loop_frames(nframes)
    orc.set_num_threads(16)
    g = capi.VisualOdometry(ctx, 1241, 376, 3, grid_step=grid_step, anms_keep=anms_keep,
                            keyframe_min_inliers=kf_min, seed=20261003)
    o = orc.VO(1241, 376, 3, grid_step=grid_step, anms_keep=anms_keep, keyframe_min_inliers=kf_min, seed=20261003)
    assert g.init(*frames[0]) == o.init(*frames[0])
    n_kf = 0
    worst_t = worst_r = 0.0
    tg_all, to_all = [], []
    for i in range(1, nframes):
        rg, Rg, tg, ig, kg, ng = g.track(*frames[i])
        ro, Ro, to, io, ko, no = o.track(*frames[i])
        assert rg == 0 and ro == 0
        assert ng == no, f"frame {i}: tracked {ng} vs {no}"
        assert ig == io, f"frame {i}: inliers {ig} vs {io}"
        assert kg == ko, f"frame {i}: keyframe decision {kg} vs {ko} at {ig} / {io} inliers"
        n_kf += kg
        dt, dr = np.linalg.norm(tg - to), float(np.abs(Rg - Ro).max())
        assert np.array_equal(tg, to) and np.array_equal(Rg, Ro), f"frame {i}: {dt:.2e} m, |dR| {dr:.2e}"
        worst_t, worst_r = max(worst_t, dt), max(worst_r, dr)
        assert np.linalg.norm(tg - poses[i][1]) < 0.02 * i + 0.05     # both follow the generator's truth
        tg_all.append(tg)
        to_all.append(to)
    a2, a3 = g.reference()
    b2, b3 = o.ref()
    assert np.array_equal(a2, b2) and np.array_equal(a3, b3)          # the reference sets too, bit for bit
    assert 0 < n_kf < nframes - 1                                     # both branches of the keyframe rule ran
    ate = float(np.sqrt(np.mean(np.sum((np.array(tg_all) - np.array(to_all)) ** 2, axis=1))))
    assert ate == 0.0
    print(f"\n{anms_keep} keypoints, {nframes - 1} frames, {n_kf} keyframes: worst pose delta vs oracle "
          f"{worst_t:.2e} m / {worst_r:.2e} rad, ATE {ate:.2e} m, every count and decision equal")
    g.close()
    o.close()


@pytest.mark.parametrize("grid_step,anms_keep,kf_min", [(30, 0, 200), (10, 4096, 2000)])
def test_frontend_matches_oracle(ctx, orc, grid_step, anms_keep, kf_min):
    nframes = 7 if grid_step == 30 else 4
    poses, frames = _frames(nframes)
    g = capi.VisualOdometry(ctx, 1241, 376, 3, grid_step=grid_step, anms_keep=anms_keep,
                            keyframe_min_inliers=kf_min, seed=5)
    o = orc.VO(1241, 376, 3, grid_step=grid_step, anms_keep=anms_keep, keyframe_min_inliers=kf_min, seed=5)
    ng, no = g.init(*frames[0]), o.init(*frames[0])
    assert ng == no
    g2, g3 = g.reference()
    o2, o3 = o.ref()
    assert np.array_equal(g2, o2)
    assert np.allclose(g3, o3, rtol=1e-5, atol=1e-5)
    saw_keyframe = False
    for i in range(1, nframes):
        rg, Rg, tg, ig, kg, ng = g.track(*frames[i])
        ro, Ro, to, io, ko, no = o.track(*frames[i])
        assert rg == 0 and ro == 0
        assert ng == no, f"frame {i}: tracked {ng} vs {no}"
        assert abs(ig - io) <= 2, f"frame {i}: inliers {ig} vs {io}"
        assert kg == ko
        saw_keyframe |= kg
        assert np.linalg.norm(tg - to) < 1e-3, f"frame {i}: dt {np.linalg.norm(tg - to)}"
        assert _rot_angle(Rg, Ro) < 1e-4
        # and both follow the generator's ground truth
        assert np.linalg.norm(tg - poses[i][1]) < 0.05
        a2, a3 = g.reference()
        b2, b3 = o.ref()
        assert a2.shape == b2.shape
        assert np.allclose(a2, b2, atol=1e-4) and np.allclose(a3, b3, rtol=1e-4, atol=1e-3)
    if grid_step == 30:
        assert saw_keyframe  # 440 grid points fall under 200 inliers within a few frames
    g.close()
    o.close()


def test_frontend_device_images_and_forced_keyframe(ctx, orc):
    import torch
    poses, frames = _frames(3)
    g = capi.VisualOdometry(ctx, 1241, 376, 3, grid_step=30, seed=1)
    o = orc.VO(1241, 376, 3, grid_step=30, seed=1)
    dev = [(torch.from_numpy(l).cuda(), torch.from_numpy(r).cuda()) for l, r in frames]
    torch.cuda.synchronize()
    assert g.init(*dev[0]) == o.init(*frames[0])
    rg, Rg, tg, ig, kg, ng = g.track(*dev[1], force_keyframe=True)   # LC_FLAG path: keyframe regardless
    ro, Ro, to, io, ko, no = o.track(*frames[1], force_keyframe=True)
    assert kg and ko and np.linalg.norm(tg - to) < 1e-3
    a2, _ = g.reference()
    b2, _ = o.ref()
    assert np.array_equal(a2, b2)
    g.close()


def test_frontend_tracking_lost(ctx):
    """Unrelated second frame: PnP finds < 10 inliers twice -> SVO_ERR_TRACKING_LOST
    (the reference's SHUTDOWN_FLAG, src/keyFrameManagement.cpp:89-92)."""
    poses, frames = _frames(1)
    g = capi.VisualOdometry(ctx, 1241, 376, 3, grid_step=30)
    g.init(*frames[0])
    rng = np.random.default_rng(0)
    junk = rng.integers(0, 256, (376, 1241, 3), dtype=np.uint8)
    rc, *_ = g.localize(junk)
    assert rc == capi.SVO_ERR_TRACKING_LOST
    g.close()


@pytest.mark.parametrize("pipeline", [False, True])
def test_run_chunk_equals_frame_by_frame(ctx, pipeline):
    """The chunk runner (optionally with the two-stream PnP / LK overlap and its speculative
    tracking) must reproduce frame-by-frame svo_vo_track exactly: poses bit for bit, the same
    keyframes, the same reference set at the end."""
    import torch
    poses, frames = _frames(9)
    dev = [(torch.from_numpy(l).cuda(), torch.from_numpy(r).cuda()) for l, r in frames]
    torch.cuda.synchronize()
    kw = dict(grid_step=30, keyframe_min_inliers=200, seed=11)
    a = capi.VisualOdometry(ctx, 1241, 376, 3, **kw)
    b = capi.VisualOdometry(ctx, 1241, 376, 3, **kw)
    assert a.init(*dev[0]) == b.init(*dev[0])
    ref = [a.track(*dev[i]) for i in range(1, 9)]
    rc, done, R, t, inl, trk, kf = b.run_chunk([d[0] for d in dev[1:]], [d[1] for d in dev[1:]], pipeline=pipeline)
    assert rc == 0 and done == 8
    assert kf.any() and not kf.all()        # both the speculation-hit and the discard path ran
    for i, (rc_i, R_i, t_i, inl_i, kf_i, trk_i) in enumerate(ref):
        assert np.array_equal(R[i], R_i) and np.array_equal(t[i], t_i), f"frame {i + 1}"
        assert inl[i] == inl_i and trk[i] == trk_i and bool(kf[i]) == kf_i
    a2, a3 = a.reference()
    b2, b3 = b.reference()
    assert np.array_equal(a2, b2) and np.array_equal(a3, b3)
    a.close()
    b.close()


@pytest.mark.parametrize("grid_step,anms_keep,kf_min", [(30, 0, 200), (10, 4096, 2000), (7, 8192, 4000)])
def test_pipelined_chunk_in_pieces_of_every_short_length(ctx, grid_step, anms_keep, kf_min):
    """The four-stream pipeline runs its pyramids and the stereo path two frames ahead and rotates buffers by frame index:
    runs of 1, 2, 3, 4 and 5 frames, one after the other on the same front-end, must hand their state over exactly --
    every pose, count and keyframe decision equal to frame-by-frame svo_vo_track, and the reference set at the end.
    At a coarse lattice and at the benchmarked shapes (4096 keypoints: the metric; 8192: configs[4])."""
    import torch
    poses, frames = _frames(17)
    dev = [(torch.from_numpy(l).cuda(), torch.from_numpy(r).cuda()) for l, r in frames]
    torch.cuda.synchronize()
    kw = dict(grid_step=grid_step, anms_keep=anms_keep, keyframe_min_inliers=kf_min, seed=11)
    a = capi.VisualOdometry(ctx, 1241, 376, 3, **kw)
    b = capi.VisualOdometry(ctx, 1241, 376, 3, **kw)
    assert a.init(*dev[0]) == b.init(*dev[0])
    pieces = [1, 2, 3, 4, 5, 1]
    assert sum(pieces) == len(dev) - 1
    ref = [a.track(*dev[i]) for i in range(1, len(dev))]
    at = 1
    kf_all = []
    for n in pieces:
        rc, done, R, t, inl, trk, kf = b.run_chunk([d[0] for d in dev[at:at + n]], [d[1] for d in dev[at:at + n]], pipeline=True)
        assert rc == 0 and done == n
        for i in range(n):
            rc_i, R_i, t_i, inl_i, kf_i, trk_i = ref[at - 1 + i]
            assert np.array_equal(R[i], R_i) and np.array_equal(t[i], t_i), f"frame {at + i}"
            assert inl[i] == inl_i and trk[i] == trk_i and bool(kf[i]) == kf_i
        kf_all.extend(bool(x) for x in kf)
        at += n
    assert any(kf_all) and not all(kf_all)
    a2, a3 = a.reference()
    b2, b3 = b.reference()
    assert np.array_equal(a2, b2) and np.array_equal(a3, b3)
    a.close()
    b.close()


def test_run_chunks_side_by_side_equals_one_by_one(ctx):
    """svo_vo_run_chunks (several chunks of the stream at once on one GPU, one context and one
    host thread each) must give every chunk exactly what svo_vo_run_chunk gives it alone."""
    import torch
    poses, frames = _frames(12)
    dev = [(torch.from_numpy(l).cuda(), torch.from_numpy(r).cuda()) for l, r in frames]
    torch.cuda.synchronize()
    kw = dict(grid_step=30, keyframe_min_inliers=200)
    chunks = [dev[0:4], dev[4:8], dev[8:12]]
    alone = []
    for k, ch in enumerate(chunks):
        v = capi.VisualOdometry(ctx, 1241, 376, 3, seed=5 + k, **kw)
        v.init(*ch[0])
        alone.append(v.run_chunk([d[0] for d in ch[1:]], [d[1] for d in ch[1:]]))
        v.close()
    ctxs = [capi.Context(0) for _ in chunks]
    vos = [capi.VisualOdometry(c, 1241, 376, 3, seed=5 + k, **kw) for k, c in enumerate(ctxs)]
    for v, ch in zip(vos, chunks):
        v.init(*ch[0])
    res = capi.run_chunks([(v, [d[0] for d in ch[1:]], [d[1] for d in ch[1:]]) for v, ch in zip(vos, chunks)])
    for one, par in zip(alone, res):
        assert one[0] == par[0] == 0 and one[1] == par[1] == 3
        for x, y in zip(one[2:], par[2:]):
            assert np.array_equal(x, y)
    with pytest.raises(capi.SvoError):  # one front-end in two jobs is refused
        capi.run_chunks([(vos[0], [], []), (vos[0], [], [])])
    for c in ctxs:
        c.close()


_SPARSE = dict(grid_step=30, keyframe_min_inliers=200)
_ANMS = dict(grid_step=10, anms_keep=4096, keyframe_min_inliers=2000)


@pytest.mark.parametrize("lengths,kw", [((4, 4, 4), _SPARSE), ((5, 3, 2, 4), _SPARSE), ((3, 2) * 8, _SPARSE),  # a full group of 16
                                        ((5, 3, 2, 4), _ANMS)],
                         ids=["lengths0", "lengths1", "lengths2", "lengths1-anms"])
def test_chunks_sharing_a_context_run_in_lock_step_with_one_lk_launch(ctx, lengths, kw):
    """Jobs whose front-ends share ONE context form a group: one host thread, one pyramidal-LK
    launch per frame for all of them (blockIdx.y = job).  Chunks of different lengths, keyframes
    falling on different frames: every chunk must still get exactly its stand-alone result -- also
    with ANMS on, whose launch then carries the group's jobs too."""
    import torch
    total = sum(lengths)
    poses, frames = _frames(total)
    dev = [(torch.from_numpy(l).cuda(), torch.from_numpy(r).cuda()) for l, r in frames]
    torch.cuda.synchronize()
    bounds, s0 = [], 0
    for n in lengths:
        bounds.append((s0, s0 + n))
        s0 += n
    alone = []
    for k, (a, b) in enumerate(bounds):
        v = capi.VisualOdometry(ctx, 1241, 376, 3, seed=20 + k, **kw)
        v.init(*dev[a])
        alone.append((v.run_chunk([d[0] for d in dev[a + 1:b]], [d[1] for d in dev[a + 1:b]], pipeline=False),
                      v.reference()))
        v.close()
    shared = capi.Context(0)
    vos = [capi.VisualOdometry(shared, 1241, 376, 3, seed=20 + k, **kw) for k in range(len(bounds))]
    jobs = []
    for v, (a, b) in zip(vos, bounds):
        v.init(*dev[a])
        jobs.append((v, [d[0] for d in dev[a + 1:b]], [d[1] for d in dev[a + 1:b]]))
    res = capi.run_chunks(jobs)
    saw_kf = False
    for (one, ref_one), par, v in zip(alone, res, vos):
        assert one[0] == par[0] == 0 and one[1] == par[1]
        for x, y in zip(one[2:], par[2:]):
            assert np.array_equal(x, y)
        saw_kf |= bool(par[6].any())
        r2, r3 = v.reference()
        assert np.array_equal(r2, ref_one[0]) and np.array_equal(r3, ref_one[1])
    assert saw_kf
    shared.close()


def test_chunk_sharded_run_against_the_sequential_one(ctx):
    """SURVEY 8e on one GPU: the stream cut into three chunks with one frame of overlap, every
    chunk re-initialised at its first frame and run side by side (svo_vo_run_chunks), the boundary
    poses prefix-composed and the chunks rebased (chunked.py -- the arithmetic the RCCL all-gather
    feeds on a multi-GPU node).  Results differ from the sequential run by construction (extra
    keyframes at chunk starts); the tolerance is on the trajectory: both stay near the generator's
    ground truth and within 5 cm of each other."""
    import torch
    from ros_stereo_slam_amd import chunked

    n = 25
    poses, frames = _frames(n, size=(620, 188))
    K4 = (359.428, 359.428, 303.5964, 92.60785)            # the KITTI intrinsics at half resolution
    dev = [(torch.from_numpy(l).cuda(), torch.from_numpy(r).cuda()) for l, r in
           [synth.Scene().stereo(R, t, K=K4, size=(620, 188))[:2] for R, t in poses]]
    torch.cuda.synchronize()
    kw = dict(grid_step=12, keyframe_min_inliers=300, seed=2, K4=K4)
    seq = capi.VisualOdometry(ctx, 620, 188, 3, **kw)
    seq.init(*dev[0])
    rc, done, R, t, *_ = seq.run_chunk([d[0] for d in dev[1:]], [d[1] for d in dev[1:]])
    assert rc == 0 and done == n - 1
    traj_seq = [np.zeros(3)] + [t[i] for i in range(n - 1)]
    bounds = chunked.chunk_bounds(n, 3)
    ctxs = [capi.Context(0) for _ in bounds]
    vos = [capi.VisualOdometry(c, 620, 188, 3, **kw) for c in ctxs]
    jobs = []
    for v, (s, e) in zip(vos, bounds):
        v.init(*dev[s])
        jobs.append((v, [d[0] for d in dev[s + 1:e + 1]], [d[1] for d in dev[s + 1:e + 1]]))
    res = capi.run_chunks(jobs)
    local = []
    for (s, e), (rc, done, Rc, tc, *_rest) in zip(bounds, res):
        assert rc == 0 and done == e - s
        local.append([(np.eye(3), np.zeros(3))] + [(Rc[i], tc[i]) for i in range(e - s)])
    starts = chunked.prefix_transforms([loc[-1] for loc in local])
    traj = []
    for k, (loc, st) in enumerate(zip(local, starts)):
        glob = chunked.rebase(loc, *st)
        traj.extend(glob if k == 0 else glob[1:])          # the overlap frame is not duplicated
    assert len(traj) == n
    gt_t = np.array([R0t for R0t in [poses[i][1] - poses[0][1] for i in range(n)]])
    ate_seq = chunked.ate_rmse(traj_seq, gt_t)
    ate_sh = chunked.ate_rmse([t for _, t in traj], gt_t)
    ate_rel = chunked.ate_rmse([t for _, t in traj], traj_seq)
    print(f"ATE vs ground truth: sequential {ate_seq:.4f} m, 3 chunks {ate_sh:.4f} m; between them {ate_rel:.4f} m")
    assert ate_seq < 0.1 and ate_sh < 0.1 and ate_rel < 0.05
    for c in ctxs:
        c.close()
    seq.close()


def test_older_vo_ladder_front_end_matches_oracle(ctx, orc):
    """svo_vo_params.policy = SVO_POLICY_VO_LADDER: visualOdometry::initSequence, src/bundleAdjust.cpp:427-548
    -- PnP-RANSAC at 4 px, a stereo keyframe on every frame, never shuts down -- frame by frame against the
    oracle's ladder (the rungs below the first are exercised on explicit point sets in
    test_gpu_pnp_anms.py::test_pnp_ladder_rungs_match_oracle)."""
    sc = synth.Scene()
    poses = synth.corridor_trajectory(6)
    frames = [sc.stereo(R, t)[:2] for R, t in poses]
    g = capi.VisualOdometry(ctx, 1241, 376, 3, grid_step=30, seed=3, policy=1)
    o = orc.VO(1241, 376, 3, grid_step=30, seed=3, policy=1)
    assert g.init(*frames[0]) == o.init(*frames[0])
    for i in range(1, 6):
        rg, Rg, tg, ig, kg, ng = g.track(*frames[i])
        ro, Ro, to, io, ko, no = o.track(*frames[i])
        assert rg == ro == 0 and kg and ko                     # every frame re-triangulates (:517-519)
        assert ng == no and abs(ig - io) <= 2 and ig >= 20, f"frame {i}: {ng}/{ig} vs {no}/{io}"
        assert np.linalg.norm(tg - to) < 1e-3 and _rot_angle(Rg, Ro) < 1e-4, f"frame {i}: {tg} vs {to}"
        assert np.linalg.norm(tg - poses[i][1]) < 0.1
        a2, a3 = g.reference()
        b2, b3 = o.ref()
        assert np.array_equal(a2, b2) and np.allclose(a3, b3, rtol=1e-4, atol=1e-3)
    with pytest.raises(capi.SvoError):                         # the chunk runner drives the live policy only
        g.run_chunk([frames[1][0]], [frames[1][1]])
    g.close()
    o.close()


@pytest.mark.parametrize("pipeline", [False, True])
def test_run_chunk_takes_the_8px_retry_on_the_host_and_resumes(ctx, orc, pipeline):
    """The chain runner keeps the host out of the frame loop; the rare slow path -- fewer than pnp_retry_below inliers
    at 1 px, PerspectiveNpointEstimation's second attempt at 8 px (src/keyFrameManagement.cpp:85-92) -- stops the
    chain on the device and is run by the host, which then queues the rest of the chunk again.  With the threshold
    raised so that many frames take it: the chunk runner == frame by frame == the oracle, bit for bit."""
    import torch
    poses, frames = _frames(10)
    dev = [(torch.from_numpy(l).cuda(), torch.from_numpy(r).cuda()) for l, r in frames]
    torch.cuda.synchronize()
    kw = dict(grid_step=30, keyframe_min_inliers=200, seed=3, pnp_retry_below=230, pnp_lost_below=10)
    a = capi.VisualOdometry(ctx, 1241, 376, 3, **kw)
    b = capi.VisualOdometry(ctx, 1241, 376, 3, **kw)
    o = orc.VO(1241, 376, 3, **kw)
    assert a.init(*dev[0]) == b.init(*dev[0]) == o.init(*frames[0])
    ref = [a.track(*dev[i]) for i in range(1, 10)]
    oref = [o.track(*frames[i]) for i in range(1, 10)]
    rc, done, R, t, inl, trk, kf = b.run_chunk([d[0] for d in dev[1:]], [d[1] for d in dev[1:]], pipeline=pipeline)
    assert rc == 0 and done == 9
    for i, ((rc_i, R_i, t_i, inl_i, kf_i, trk_i), (rc_o, R_o, t_o, inl_o, kf_o, trk_o)) in enumerate(zip(ref, oref)):
        assert rc_i == 0 and rc_o == 0
        assert np.array_equal(R[i], R_i) and np.array_equal(t[i], t_i), f"frame {i + 1} vs frame by frame"
        assert np.array_equal(R[i], R_o) and np.array_equal(t[i], t_o), f"frame {i + 1} vs oracle"
        assert inl[i] == inl_i == inl_o and trk[i] == trk_i == trk_o and bool(kf[i]) == kf_i == bool(kf_o)
    a2, a3 = a.reference()
    b2, b3 = b.reference()
    o2, o3 = o.ref()
    assert np.array_equal(a2, b2) and np.array_equal(a3, b3) and np.array_equal(b2, o2) and np.array_equal(b3, o3)
    # the 1 px attempt of a 440-point grid finds fewer than 230 inliers on most frames: the slow path really ran
    plain = capi.VisualOdometry(ctx, 1241, 376, 3, grid_step=30, keyframe_min_inliers=200, seed=3)
    plain.init(*dev[0])
    counts = [plain.track(*dev[i])[3] for i in range(1, 10)]
    assert sum(c < 230 for c in counts) >= 3
    for v in (a, b, plain):
        v.close()
    o.close()


def test_lock_step_group_with_a_chunk_on_the_slow_path(ctx):
    """A lock-step group in which ONE chunk takes the host's retry path: that chunk is finished on its own after the
    others, every chunk still gets its stand-alone result."""
    import torch
    poses, frames = _frames(12)
    dev = [(torch.from_numpy(l).cuda(), torch.from_numpy(r).cuda()) for l, r in frames]
    torch.cuda.synchronize()
    bounds = [(0, 4), (4, 8), (8, 12)]
    kws = [dict(grid_step=30, keyframe_min_inliers=200, seed=40 + k, pnp_retry_below=230 if k == 1 else 10) for k in range(3)]
    alone = []
    for kw, (a, b) in zip(kws, bounds):
        v = capi.VisualOdometry(ctx, 1241, 376, 3, **kw)
        v.init(*dev[a])
        ref = [v.track(*dev[i]) for i in range(a + 1, b)]
        alone.append((ref, v.reference()))
        v.close()
    shared = capi.Context(0)
    vos = [capi.VisualOdometry(shared, 1241, 376, 3, **kw) for kw in kws]
    jobs = []
    for v, (a, b) in zip(vos, bounds):
        v.init(*dev[a])
        jobs.append((v, [d[0] for d in dev[a + 1:b]], [d[1] for d in dev[a + 1:b]]))
    res = capi.run_chunks(jobs)
    for (ref, ref_sets), (rc, done, R, t, inl, trk, kf), v in zip(alone, res, vos):
        assert rc == 0 and done == len(ref)
        for i, (rc_i, R_i, t_i, inl_i, kf_i, trk_i) in enumerate(ref):
            assert np.array_equal(R[i], R_i) and np.array_equal(t[i], t_i)
            assert inl[i] == inl_i and trk[i] == trk_i and bool(kf[i]) == kf_i
        r2, r3 = v.reference()
        assert np.array_equal(r2, ref_sets[0]) and np.array_equal(r3, ref_sets[1])
    shared.close()


@pytest.mark.parametrize("pipeline", [False, True])
def test_run_chunk_reports_tracking_lost_in_the_middle_of_a_chunk(ctx, pipeline):
    """An unrelated image in the middle of a chunk: the chain halts there on the device, the host's retry fails too ->
    SVO_ERR_TRACKING_LOST with n_done = the frames before it, their results intact (SHUTDOWN_FLAG,
    src/keyFrameManagement.cpp:89-92)."""
    import torch
    poses, frames = _frames(6)
    rng = np.random.default_rng(0)
    junk = rng.integers(0, 256, (376, 1241, 3), dtype=np.uint8)
    frames = frames[:4] + [(junk, junk)] + frames[4:]
    dev = [(torch.from_numpy(l).cuda(), torch.from_numpy(r).cuda()) for l, r in frames]
    torch.cuda.synchronize()
    kw = dict(grid_step=30, keyframe_min_inliers=200, seed=2)
    a = capi.VisualOdometry(ctx, 1241, 376, 3, **kw)
    b = capi.VisualOdometry(ctx, 1241, 376, 3, **kw)
    a.init(*dev[0])
    b.init(*dev[0])
    ref = [a.track(*dev[i]) for i in range(1, 4)]
    assert a.track(*dev[4])[0] == capi.SVO_ERR_TRACKING_LOST
    rc, done, R, t, inl, trk, kf = b.run_chunk([d[0] for d in dev[1:]], [d[1] for d in dev[1:]], pipeline=pipeline)
    assert rc == capi.SVO_ERR_TRACKING_LOST and done == 3
    for i, (rc_i, R_i, t_i, inl_i, kf_i, trk_i) in enumerate(ref):
        assert np.array_equal(R[i], R_i) and np.array_equal(t[i], t_i) and inl[i] == inl_i and bool(kf[i]) == kf_i
    a.close()
    b.close()


@pytest.mark.parametrize("host_pipeline", [False, True])
def test_run_chunk_takes_host_images(ctx, host_pipeline):
    """Host images go through the serial runner's upload ring, in order: the same results as device images.  Asking for
    the pipeline with host images falls back to the serial runner: the same results as pipeline=False."""
    import torch
    poses, frames = _frames(6)
    dev = [(torch.from_numpy(l).cuda(), torch.from_numpy(r).cuda()) for l, r in frames]
    torch.cuda.synchronize()
    kw = dict(grid_step=30, keyframe_min_inliers=200, seed=8)
    a = capi.VisualOdometry(ctx, 1241, 376, 3, **kw)
    b = capi.VisualOdometry(ctx, 1241, 376, 3, **kw)
    a.init(*dev[0])
    b.init(*frames[0])
    ra = a.run_chunk([d[0] for d in dev[1:]], [d[1] for d in dev[1:]], pipeline=True)
    rb = b.run_chunk([f[0] for f in frames[1:]], [f[1] for f in frames[1:]], pipeline=host_pipeline)
    assert ra[0] == rb[0] == 0 and ra[1] == rb[1] == 5
    for x, y in zip(ra[2:], rb[2:]):
        assert np.array_equal(x, y)
    if host_pipeline:
        c = capi.VisualOdometry(ctx, 1241, 376, 3, **kw)
        c.init(*frames[0])
        rc = c.run_chunk([f[0] for f in frames[1:]], [f[1] for f in frames[1:]], pipeline=False)
        assert rc[0] == 0 and rc[1] == 5
        for x, y in zip(rb[2:], rc[2:]):
            assert np.array_equal(x, y)
        c.close()
    a.close()
    b.close()


def test_lock_step_groups_take_host_images_through_the_upload_ring(ctx):
    """Chunks that share a context with their frames in HOST memory (KITTI replay): the library uploads step f + 2 on a copy
    stream while step f computes (a ring of three slots) -- pageable numpy arrays and pinned torch tensors give what device
    images give, bit for bit; chunks of different lengths; the chunks initialise inside the call."""
    import torch
    poses, frames = _frames(14)
    dev = [(torch.from_numpy(l).cuda(), torch.from_numpy(r).cuda()) for l, r in frames]
    pinned = [(torch.from_numpy(l).pin_memory(), torch.from_numpy(r).pin_memory()) for l, r in frames]
    torch.cuda.synchronize()
    kw = dict(grid_step=30, keyframe_min_inliers=200)
    spans = [(0, 6), (3, 13), (7, 9)]

    def run(src, shared):
        vos = [capi.VisualOdometry(shared, 1241, 376, 3, seed=4 + k, **kw) for k in range(3)]
        res = capi.run_chunks([(v, [f[0] for f in src[s:e + 1]], [f[1] for f in src[s:e + 1]]) for v, (s, e) in zip(vos, spans)],
                              pipeline=False, init=True)
        for v in vos:
            v.close()
        return res

    ctxs = [capi.Context(0) for _ in range(3)]
    ref, host, pin = run(dev, ctxs[0]), run(frames, ctxs[1]), run(pinned, ctxs[2])
    for got in (host, pin):
        for x, y in zip(ref, got):
            assert x[0] == y[0] == 0 and x[1] == y[1]
            for p, q in zip(x[2:], y[2:]):
                assert np.array_equal(p, q)
    assert [r[1] for r in ref] == [6, 10, 2]
    with pytest.raises(capi.SvoError):       # one group, images from both sides: refused
        a, b = capi.VisualOdometry(ctxs[0], 1241, 376, 3, **kw), capi.VisualOdometry(ctxs[0], 1241, 376, 3, **kw)
        capi.run_chunks([(a, [f[0] for f in dev[:3]], [f[1] for f in dev[:3]]), (b, [f[0] for f in frames[:3]], [f[1] for f in frames[:3]])],
                        pipeline=False, init=True)
    for c in ctxs:
        c.close()


def test_keyframe_colors_on_the_fused_path(ctx, orc):
    """`colors` of stereoTriangulate (getColors(imL, x1): B, G, R floats, include/monoUtils.h:180-193) come out of the
    fused path's triangulation launch, point for point with the keyframe's 2-D set -- at initialisation, at a forced
    keyframe and at the keyframes of a pipelined chunk (what src/VisualSLAM.cpp:125-136 pushes into colorHistory)."""
    import torch
    poses, frames = _frames(8)
    rng = np.random.default_rng(3)
    frames = [(np.ascontiguousarray(l + rng.integers(0, 3, l.shape, dtype=np.uint8) * np.array([0, 2, 4], np.uint8)), r)
              for l, r in frames]           # channels that differ, so that B / G / R order matters
    dev = [(torch.from_numpy(l).cuda(), torch.from_numpy(r).cuda()) for l, r in frames]
    torch.cuda.synchronize()
    g = capi.VisualOdometry(ctx, 1241, 376, 3, grid_step=30, keyframe_min_inliers=200, seed=4)
    n0 = g.init(*dev[0])
    ref2d, _ = g.reference()
    col = g.keyframe_colors()
    assert col.shape == (n0, 3) and np.array_equal(col, orc.get_colors(frames[0][0], ref2d))
    rc, R, t, inl, kf, trk = g.track(*dev[1], force_keyframe=True)
    assert rc == 0 and kf
    ref2d, _ = g.reference()
    assert np.array_equal(g.keyframe_colors(), orc.get_colors(frames[1][0], ref2d))
    rc, done, R, t, inl, trk, kfs = g.run_chunk([d[0] for d in dev[2:]], [d[1] for d in dev[2:]], pipeline=True)
    assert rc == 0 and kfs.any()
    last_kf = 2 + int(np.nonzero(kfs)[0][-1])
    col = g.keyframe_colors()
    assert len(col) == len(g.keyframe_cloud())
    if kfs[-1]:     # the reference set is still the keyframe's: compare point for point
        ref2d, _ = g.reference()
        assert np.array_equal(col, orc.get_colors(frames[last_kf][0], ref2d))
    else:           # colours are pixel values of that keyframe's left image
        assert set(np.unique(col)).issubset(set(np.unique(frames[last_kf][0]).astype(np.float32)))
    g.close()


def test_pipeline_soak_600_frames_in_pieces_of_random_length(ctx):
    """the four-stream pipeline's hazards are timing-dependent (buffers and events indexed by f & 1, f % 3,
    g & 3, shared by streams that run two frames ahead), so its race coverage must not live in a tool only.  One round of
    tools/pipeline_soak.py: 600 frames of the benchmark stream at the benchmarked shape through the pipelined runner in
    pieces of random length (1 .. 89) against the one-stream runner on a second context -- every pose, count and
    keyframe decision and the final reference sets bit for bit.  A later edit that breaks a buffer rotation shows here."""
    import torch

    n = 600
    rng = np.random.default_rng(1)
    poses = synth.loop_trajectory(n + 1, **synth.BENCH_LOOP)
    lefts, rights = synth.stereo_torch(synth.bench_scene(), poses, device="cuda", batch=8)
    torch.cuda.synchronize()
    kw = dict(grid_step=10, anms_keep=4096, keyframe_min_inliers=2000, seed=20261003)
    other = capi.Context(0)
    a = capi.VisualOdometry(ctx, 1241, 376, 3, **kw)
    b = capi.VisualOdometry(other, 1241, 376, 3, **kw)
    assert a.init(lefts[0], rights[0]) == b.init(lefts[0], rights[0])
    at, kfs, pieces = 1, 0, 0
    while at <= n:
        m = int(min(n + 1 - at, rng.integers(1, 90)))
        ra = a.run_chunk(list(lefts[at:at + m]), list(rights[at:at + m]), pipeline=True)
        rb = b.run_chunk(list(lefts[at:at + m]), list(rights[at:at + m]), pipeline=False)
        assert ra[0] == rb[0] == 0 and ra[1] == rb[1] == m, (ra[0], rb[0], ra[1], rb[1], at)
        for k in range(2, 7):
            assert np.array_equal(ra[k], rb[k]), f"output {k} differs in the piece of {m} frames from frame {at}"
        kfs += int(ra[6].sum())
        at += m
        pieces += 1
    a2, a3 = a.reference()
    b2, b3 = b.reference()
    assert np.array_equal(a2, b2) and np.array_equal(a3, b3)
    assert 100 < kfs < n - 100 and pieces > 8
    a.close()
    b.close()
    other.close()
