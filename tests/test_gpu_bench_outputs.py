"""bench.py's plain run and ``--dump-outputs``: the line carries the headline keys and nothing that takes a run of its
own, the outputs of the last timed step are written as float64 ``.npy`` and are the same on every run with the same
arguments; the stream that renders each distinct pose once is the stream ``synth.stereo_torch`` renders."""
import json
import os
import pathlib
import subprocess
import sys
from unittest import mock

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]


SHAPES = {"last_step_R": (64, 3, 3), "last_step_t": (64, 3), "last_step_inliers": (64,), "last_step_tracked": (64,),
          "last_step_keyframe": (64,), "chunk_start_R": (64, 3, 3), "chunk_start_t": (64, 3)}


def plain_run(out_dir, steps, warmup):
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                        "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.lstrip().startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["metric"] == "stereo frames/sec @1241x376, 4096 kpts" and d["unit"] == "frames/s"
    assert d["higher_is_better"] is True and d["steps"] == steps and d["repeats"] == 1
    # one clock over the K steps: ms_per_step, the timed total and value all come from it
    assert d["timed_s_total"] == pytest.approx(d["ms_per_step"] * steps / 1e3)
    assert d["value"] == pytest.approx(64 * steps / d["timed_s_total"])
    assert not {"roofline", "cpu_baseline", "kpts8192", "posegraph", "single_chunk_frames_per_s"} & d.keys()
    assert sorted(os.listdir(out_dir)) == sorted(f"{n}.npy" for n in SHAPES)
    assert sum(f.stat().st_size for f in out_dir.iterdir()) < 64 << 20
    out = {n: np.load(out_dir / f"{n}.npy") for n in SHAPES}
    for n, shape in SHAPES.items():
        assert out[n].dtype == np.float64 and out[n].shape == shape and np.isfinite(out[n]).all(), n
    return d, out


@pytest.mark.gpu
def test_plain_run_line_and_outputs_of_the_last_step(tmp_path):
    from ros_stereo_slam_amd import chunked, synth

    # 64 chunks of L = 9 frames: 577 frames, past the 492-frame lap, so repeated poses are in the stream
    L = 9
    d1, o1 = plain_run(tmp_path / "a", 8, 1)
    d2, o2 = plain_run(tmp_path / "b", 8, 1)
    assert d1["ate_rmse_vs_truth"] == d2["ate_rmse_vs_truth"]
    for n in SHAPES:
        assert np.array_equal(o1[n], o2[n]), n
    # the last step is every chunk's boundary frame: the exchange composed the chunk starts from exactly these poses
    R, t, sR, st = o1["last_step_R"], o1["last_step_t"], o1["chunk_start_R"], o1["chunk_start_t"]
    assert np.array_equal(sR[0], np.eye(3)) and np.array_equal(st[0], np.zeros(3))
    for m in range(63):
        Rn, tn = chunked.compose(sR[m].copy(), st[m].copy(), R[m].copy(), t[m].copy())
        assert np.allclose(Rn, sR[m + 1], rtol=0, atol=1e-9) and np.allclose(tn, st[m + 1], rtol=0, atol=1e-9), m
    # ... and it is frame W + K of the chunk, not an earlier one: the generator's pose of that frame relative to the
    # chunk's first frame is within a few cm (one frame earlier is 0.9 m away)
    poses = synth.loop_trajectory(64 * L + 1, **synth.BENCH_LOOP)
    for m in range(64):
        (Rs, ts), (Re, te), (Rp, tp) = poses[m * L], poses[(m + 1) * L], poses[(m + 1) * L - 1]
        assert np.linalg.norm(t[m] - Rs.T @ (te - ts)) < 0.1, m
        assert np.linalg.norm(t[m] - Rs.T @ (tp - ts)) > 0.5, m
        assert np.abs(R[m] - Rs.T @ Re).max() < 0.01, m
    assert o1["last_step_tracked"].min() > 0 and o1["last_step_inliers"].min() > 0
    # the same frames split as 2 warm-up + 7 timed steps: the same outputs, the line counts 7 steps
    d3, o3 = plain_run(tmp_path / "c", 7, 2)
    assert d3["config"]["frames_per_chunk"] == L
    for n in SHAPES:
        assert np.array_equal(o1[n], o3[n]), n


@pytest.mark.gpu
def test_render_stream_equals_stereo_torch():
    import torch

    from ros_stereo_slam_amd import synth

    with mock.patch.dict(os.environ):   # bench.py sets GPU_MAX_HW_QUEUES for its own process
        sys.path.insert(0, str(ROOT))
        import bench
    poses = synth.loop_trajectory(510, **synth.BENCH_LOOP)
    # the first lap's end, the lap boundary inside one batch, repeats of the start in batches of their own
    sel = poses[480:500] + poses[0:12] + poses[492:502]
    scene = synth.bench_scene()
    ref_l, ref_r = synth.stereo_torch(scene, sel, device="cuda", batch=8)
    got_l, got_r = bench.render_stream(scene, sel, device="cuda", batch=8)
    assert len(got_l) == len(got_r) == len(sel)
    assert all(torch.equal(a, b) for a, b in zip(ref_l + ref_r, got_l + got_r))
