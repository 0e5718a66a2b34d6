"""The loop detector on the GPU (loopdet.hip, bow.hip) against the oracle at every setting of tests/loopdet_fixtures.py's table --
tests/test_loopdet_params.py proves on the CPU that each of them changes decisions and which.  Both are fed the same features.
Frame by frame: the candidates of the database query in order, their scores and the normalisation score bit for bit, the status
and the match; in every submission form, since each forms its verdicts in code of its own: one frame at a time, the whole stream
in groups of 16 (or of `dislocal`), and a filled prefix followed by the rest."""
import gc
import weakref

import numpy as np
import pytest

import loopdet_fixtures as lf
from ros_stereo_slam_amd import capi

pytestmark = pytest.mark.gpu
W, H = lf.SIZE
FILL = 37          # the prefix that is filled, not queried: past dislocal, no multiple of a group of 16


@pytest.fixture(scope="module")
def setup(ctx, orc):
    imgs, feats, ov = lf.stream()
    a = ov.arrays()
    gv = capi.Vocabulary.from_arrays(ctx, ov.k, ov.L, a["parent"], a["desc"], a["weight"])
    own = capi.Context(0)
    yield dict(imgs=imgs, feats=feats, packed=lf.pack(feats), gv=gv, own=own)
    gv.close()
    own.close()


def _detector(c, setup, entry):
    det = capi.LoopDetector(c, W, H, 3, **entry.lib_params())
    if entry.voc:
        det.set_vocabulary(setup["gv"], entry.di_levels)
    return det


def _same(got, want, form):
    """one frame: the library's collect_ex against the oracle's record"""
    i = want["query"]
    assert got["query"] == i, form
    assert got["cand_id"].tolist() == want["cand_id"], (form, i, got["cand_id"].tolist(), want["cand_id"])
    assert np.array_equal(got["cand_score"], np.array(want["cand_score"])), (form, i)
    assert not want["cand_id"] or got["ns_factor"] == want["ns"], (form, i, got["ns_factor"], want["ns"])
    assert got["status"] == want["status"], (form, i, lf.STATUS[got["status"]], lf.STATUS[want["status"]])
    assert got["match"] == want["match"], (form, i, got["match"], want["match"])


@pytest.mark.parametrize("entry", [lf.DEFAULT] + lf.TABLE, ids=repr)
def test_one_frame_at_a_time(ctx, setup, entry):
    want = lf.run_oracle(entry)
    det = _detector(ctx, setup, entry)
    for (xy, desc), w in zip(setup["feats"], want):
        det.submit_features(xy, desc)
        _same(det.collect_ex(), w, "submit_features")
    det.close()


@pytest.mark.parametrize("entry", [lf.DEFAULT] + lf.TABLE, ids=repr)
def test_the_whole_stream_in_groups(ctx, setup, entry):
    want = lf.run_oracle(entry)
    det = _detector(setup["own"], setup, entry)
    det.submit_features_batch(*setup["packed"])
    assert det.pending() == len(want)
    for w in want:
        _same(det.collect_ex(), w, "submit_features_batch")
    assert det.pending() == 0
    det.close()


@pytest.mark.parametrize("entry", [lf.DEFAULT] + lf.TABLE, ids=repr)
def test_a_filled_prefix_then_the_rest(ctx, setup, entry):
    want = lf.run_oracle(entry, fill=FILL)
    fn, fxy, fdesc = setup["packed"]
    det = _detector(setup["own"], setup, entry)
    det.fill_features_batch(fn[:FILL], fxy[:FILL], fdesc[:FILL])
    assert det.pending() == 0 and len(det) == FILL
    det.submit_features_batch(fn[FILL:], fxy[FILL:], fdesc[FILL:])
    assert want[0]["query"] == FILL
    for w in want:
        _same(det.collect_ex(), w, "fill_features_batch + submit_features_batch")
    det.close()


def test_two_settings_on_one_context_share_nothing(ctx, setup):
    """Detectors of different settings on the same context, one after the other and side by side: each gives the verdicts of the
    oracle's fresh run -- no window, database or parameter of one shows in another."""
    first, second = lf.BY_NAME["k3_loose_short_chains_never_pass"], lf.BY_NAME["dislocal_16_queries_from_frame_17"]
    a = _detector(ctx, setup, first)
    a.submit_features_batch(*setup["packed"])
    for w in lf.run_oracle(first):
        _same(a.collect_ex(), w, "first setting")
    b = _detector(ctx, setup, second)               # while the first detector, its database full, is still alive
    c = _detector(ctx, setup, first)
    for (xy, desc), wb, wc in zip(setup["feats"], lf.run_oracle(second), lf.run_oracle(first)):
        b.submit_features(xy, desc)
        c.submit_features(xy, desc)
        _same(b.collect_ex(), wb, "second setting")
        _same(c.collect_ex(), wc, "first setting again, interleaved")
    for d in (a, b, c):
        d.close()


def test_out_of_range_parameters_are_refused(ctx):
    import ctypes as C

    def create(**kw):
        prm = capi.LcParams()
        ctx.lib.svo_lc_default_params(C.byref(prm))
        for k, v in kw.items():
            setattr(prm, k, v)
        h = C.c_void_p(0xdead)
        return ctx.lib.svo_lc_create(ctx._h, C.byref(prm), W, H, 3, C.byref(h)), h.value

    SVO_ERR_ARG = -1
    for bad in (dict(k=-1), dict(alpha=-0.01), dict(alpha=1.5), dict(alpha=float("nan")), dict(dislocal=-1),
                dict(max_db_results=65), dict(max_db_results=0)):
        assert create(**bad) == (SVO_ERR_ARG, None), bad
        with pytest.raises(capi.SvoError):
            capi.LoopDetector(ctx, W, H, 3, **bad)
    for good in (dict(k=0), dict(alpha=0.0), dict(alpha=1.0), dict(dislocal=0), dict(max_db_results=64)):   # the edges themselves
        rc, h = create(**good)
        assert rc == 0 and h, good
        assert ctx.lib.svo_lc_destroy(C.c_void_p(h)) == 0


def test_submitted_images_are_held_until_their_frames_are_collected(ctx, setup):
    """The queued work reads the caller's device images: every submission's images stay referenced by the detector until
    collect has passed its last frame -- not merely until the next submission -- and are let go then.  Host images are read
    as contiguous uint8 whatever their layout."""
    import torch

    imgs = setup["imgs"]
    det = capi.LoopDetector(setup["own"], W, H, 3, seed=lf.SEED)
    det.set_vocabulary(setup["gv"], 2)
    first = [torch.from_numpy(im).cuda() for im in imgs[:18]]
    refs = [weakref.ref(t) for t in first]
    det.submit_batch(first)
    del first
    det.submit_batch([torch.from_numpy(im).cuda() for im in imgs[18:24]])
    one = torch.from_numpy(imgs[24]).cuda()
    ref_one = weakref.ref(one)
    det.submit(one)
    del one
    gc.collect()
    assert all(r() is not None for r in refs) and ref_one() is not None
    for _ in range(17):
        det.collect()
    gc.collect()
    assert all(r() is not None for r in refs)            # frame 17 of the first submission is still queued
    det.collect()
    gc.collect()
    assert all(r() is None for r in refs) and ref_one() is not None
    assert len(det.collect_batch(6)) == 6 and ref_one() is not None
    det.collect_ex()
    gc.collect()
    assert ref_one() is None and det.pending() == 0 and not det._keep_images
    det.close()
    # host images of another layout and type: the bytes of the uint8 image
    a = capi.LoopDetector(ctx, W, H, 3, seed=lf.SEED, dislocal=0)
    b = capi.LoopDetector(ctx, W, H, 3, seed=lf.SEED, dislocal=0)
    for im in imgs[:3]:
        a.submit(im)
        b.submit(np.asfortranarray(im.astype(np.int64)))
        x, y = a.collect_ex(), b.collect_ex()
        assert x["status"] == y["status"] and np.array_equal(x["cand_score"], y["cand_score"]) and x["cand_id"].tolist() == y["cand_id"].tolist()
    assert len(y["cand_id"]) == 2
    b.submit_batch([np.asfortranarray(im) for im in imgs[3:5]])
    a.submit_batch(imgs[3:5])
    assert [a.collect() for _ in range(2)] == [b.collect() for _ in range(2)]
    a.close()
    b.close()
