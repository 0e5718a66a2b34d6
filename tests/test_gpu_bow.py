"""The bag-of-words side of the loop detector on the GPU (bow.hip, loopdet.hip in vocabulary mode) against its oracle
(oracle/bow.c, oracle/loop_detector.py): the trained tree node for node, words / weights / BowVectors bit for bit, and the
detector frame by frame -- the candidates of the database query, their L1 scores, the normalisation score and the verdict
of DLoopDetector::detectLoop (include/TemplatedLoopDetector.h:696-861) with the reference's parameters
(include/visualSLAM.h:120-127: use_nss, alpha 0.9, k 1, GEOM_DI, di_levels 2) and the reference trainer's shape
(src/bagOfWordsDetector.cpp:46-56: k 9, L 6, TF_IDF, L1_NORM)."""
import numpy as np
import pytest

from bow_fixtures import noisy_descriptor_images
from oracle import orc
from oracle.loop_detector import LoopDetector as OracleDetector, Params
from ros_stereo_slam_amd import capi, synth, vocabulary

pytestmark = pytest.mark.gpu
SIZE, K4 = (480, 160), (270.0, 270.0, 240.0, 80.0)


def _same_tree(g, o):
    ga, oa = g.arrays(), o.arrays()
    assert g.n_nodes == o.n_nodes and g.n_words == o.n_words, (g.n_nodes, o.n_nodes, g.n_words, o.n_words)
    assert np.array_equal(ga["parent"], oa["parent"])
    assert np.array_equal(ga["desc"], oa["desc"])
    assert np.array_equal(ga["word_id"], oa["word_id"])
    assert np.array_equal(ga["weight"], oa["weight"])          # idf through the shared svo_log: the same bits


@pytest.mark.parametrize("k,L,seed", [(9, 4, 3), (9, 6, 11), (4, 3, 0), (10, 2, 7)])
def test_training_builds_the_oracles_tree_node_for_node(ctx, k, L, seed):
    imgs = noisy_descriptor_images(n_images=30, per_image=260, n_proto=150, seed=seed)
    g = capi.Vocabulary.train(ctx, imgs, k=k, L=L, seed=seed)
    o = orc.Vocabulary.train(imgs, k=k, L=L, seed=seed)
    assert g.k == k and g.L == L
    _same_tree(g, o)
    for im in imgs[:4]:
        for levelsup in (0, 2):
            for a, b in zip(g.transform(im, levelsup), o.transform(im, levelsup)):
                assert np.array_equal(a, b)
            for a, b in zip(g.bow(im, levelsup), o.bow(im, levelsup)):
                assert np.array_equal(a, b)
    g.close()


def test_training_edge_cases(ctx):
    rng = np.random.default_rng(1)
    one = [rng.integers(0, 2 ** 32, (1, 8), dtype=np.uint64).astype(np.uint32)]                 # a single descriptor
    same = [np.repeat(one[0], 40, axis=0), np.repeat(one[0], 25, axis=0)]                         # all identical: kmeans++ stops at one centre
    few = [rng.integers(0, 2 ** 32, (5, 8), dtype=np.uint64).astype(np.uint32)]                  # fewer than k
    for imgs in (one, same, few):
        g = capi.Vocabulary.train(ctx, imgs, k=9, L=3, seed=2)
        o = orc.Vocabulary.train(imgs, k=9, L=3, seed=2)
        _same_tree(g, o)
        for a, b in zip(g.bow(imgs[0], 1), o.bow(imgs[0], 1)):
            assert np.array_equal(a, b)
        g.close()
    with pytest.raises(capi.SvoError):
        capi.Vocabulary.train(ctx, few, k=40, L=3)


def _loop_images(n=134):
    poses = synth.loop_trajectory(n, half_x=6, half_z=10, radius=4, step=0.5)
    sc = synth.Scene(wall_x=14, z_min=-18, z_max=18)
    return poses, [sc.stereo(R, t, K=K4, size=SIZE)[0] for R, t in poses]


def _features(ctx, imgs):
    return ctx.orb_extract_batch(imgs)       # cv::ORB's own shape, the detector's default: (xy, octave, response, dir, desc)


@pytest.fixture(scope="module")
def loop_setup(ctx):
    poses, imgs = _loop_images()
    feats = _features(ctx, imgs)
    train = [f[4] for f in feats[::2]]                       # every second frame trains the vocabulary (k 9, L 6)
    g = capi.Vocabulary.train(ctx, train, k=9, L=6, seed=20261003)
    o = orc.Vocabulary.train(train, k=9, L=6, seed=20261003)
    return poses, imgs, feats, g, o


def test_vocabulary_of_real_orb_descriptors_and_the_file_format(ctx, loop_setup, tmp_path):
    poses, imgs, feats, g, o = loop_setup
    _same_tree(g, o)
    assert g.n_words > 5000
    a = g.arrays()
    vocabulary.save_dbow2(tmp_path / "orb_voc.yml.gz", g.k, g.L, a["parent"], a["desc"], a["weight"], a["word_id"])
    f = vocabulary.load_dbow2(tmp_path / "orb_voc.yml.gz")
    g2 = capi.Vocabulary.from_arrays(ctx, f["k"], f["L"], f["parent"], f["desc"], f["weight"])
    assert g2.n_words == g.n_words
    for xy, octv, resp, d, desc in feats[1:6]:
        for x, y in zip(g2.bow(desc, 2), o.bow(desc, 2)):
            assert np.array_equal(x, y)
    g2.close()


@pytest.mark.parametrize("alpha", [0.9, 0.3])
def test_bow_detector_matches_oracle_frame_by_frame(ctx, loop_setup, alpha):
    """Every frame: the candidates of the database query (ids in order), their scores, the normalisation score, the status
    and the matched entry.  Scores are compared to 1e-12 -- and found EQUAL: the GPU adds an entry's terms in
    word order, as queryL1's map does."""
    poses, imgs, feats, gv, ov = loop_setup
    g = capi.LoopDetector(ctx, SIZE[0], SIZE[1], 3, alpha=alpha, seed=5)
    g.set_vocabulary(gv, 2)
    o = OracleDetector(Params(alpha=alpha, seed=5), voc=ov, di_levels=2)
    accepted_g, accepted_o, worst, n_equal, n_cmp = [], [], 0.0, 0, 0
    for i, img in enumerate(imgs):
        g.submit(img)
        rg = g.collect_ex()
        ro = o.detect(img)
        ids_o, sc_o, ns_o = o.last_query
        assert rg["query"] == ro["query"] == i
        assert rg["cand_id"].tolist() == ids_o, (i, rg["cand_id"].tolist(), ids_o)
        if len(ids_o):
            worst = max(worst, float(np.abs(rg["cand_score"] - np.array(sc_o)).max()), abs(rg["ns_factor"] - ns_o))
            n_equal += int(np.array_equal(rg["cand_score"], np.array(sc_o)) and rg["ns_factor"] == ns_o)
            n_cmp += 1
            assert (np.diff(rg["cand_score"]) <= 0).all() and 0.0 <= rg["cand_score"].min() and rg["cand_score"].max() <= 1.0 + 1e-12
        assert rg["status"] == ro["status"], (i, capi.LC_STATUS[rg["status"]], capi.LC_STATUS[ro["status"]])
        assert rg["match"] == ro["match"], i
        for r, acc in ((rg, accepted_g), (ro, accepted_o)):
            if r["status"] == 0 and r["query"] - r["match"] > 100:      # src/optimizationStuff.cpp:58
                acc.append((r["query"], r["match"]))
    assert worst <= 1e-12 and n_cmp > 80
    assert n_equal == n_cmp, f"{n_equal} of {n_cmp} frames bit-equal, worst difference {worst:.2e}"
    assert accepted_g == accepted_o and accepted_g
    gt = synth.loop_closures(poses, min_gap=100)
    first_true = next(i for i, m in enumerate(gt) if m >= 0)
    q, m = accepted_g[0]
    assert abs(q - first_true) <= 8 and m <= 8
    g.close()


def test_another_feature_budget_in_groups_of_sixteen_matches_the_oracle(ctx, loop_setup):
    """200 features per frame instead of 500: the per-entry row masks of the query sums are 8 words instead of 16, the
    BowVector kernel's LDS and the match kernel's slots follow the budget -- the batched detector (16 frames per set of
    launches, checks on the device) against the oracle's detector frame by frame: candidates, scores, verdicts."""
    poses, imgs, feats, gv, ov = loop_setup
    own = capi.Context(0)
    g = capi.LoopDetector(own, SIZE[0], SIZE[1], 3, seed=5, n_features=200)
    g.set_vocabulary(gv, 2)
    o = OracleDetector(Params(seed=5, n_features=200), voc=ov, di_levels=2)
    g.submit_batch(imgs)
    n_det = n_geo = 0
    for i, img in enumerate(imgs):
        rg, ro = g.collect_ex(), o.detect(img)
        ids_o, sc_o, ns_o = o.last_query
        assert rg["cand_id"].tolist() == ids_o, i
        assert np.array_equal(rg["cand_score"], np.array(sc_o)) and (not ids_o or rg["ns_factor"] == ns_o), i
        assert (rg["status"], rg["match"]) == (ro["status"], ro["match"]), (i, capi.LC_STATUS[rg["status"]], capi.LC_STATUS[ro["status"]])
        n_det += ro["status"] == 0
        n_geo += ro["status"] in (0, 7)
    assert n_geo > 10 and n_det > 0, (n_geo, n_det)
    g.close()
    own.close()


def test_features_submitted_from_elsewhere_and_queued(ctx, loop_setup):
    """svo_lc_submit_features (a chunk-sharded run: ORB on the rank that holds the images, the database on rank 0): the
    verdicts of the image form; all frames queued before the first is collected."""
    poses, imgs, feats, gv, ov = loop_setup
    own = capi.Context(0)
    a = capi.LoopDetector(ctx, SIZE[0], SIZE[1], 3, seed=5)
    b = capi.LoopDetector(own, SIZE[0], SIZE[1], 3, seed=5)
    a.set_vocabulary(gv, 2)
    b.set_vocabulary(gv, 2)
    ref = []
    for img in imgs:
        a.submit(img)
        ref.append(a.collect())
    for xy, octv, resp, d, desc in feats:
        b.submit_features(xy, desc)
    assert b.pending() == len(feats)
    assert [b.collect() for _ in feats] == ref
    assert any(r["status"] == 0 for r in ref)
    # and without a vocabulary (the vocabulary-free similarity of rounds 2-3)
    c = capi.LoopDetector(ctx, SIZE[0], SIZE[1], 3, seed=5)
    d_ = capi.LoopDetector(own, SIZE[0], SIZE[1], 3, seed=5)
    for img, f in zip(imgs[:60], feats[:60]):
        d_.submit_features(f[0], f[4])
        assert c.detect(img) == d_.collect()
    with pytest.raises(capi.SvoError):
        c.set_vocabulary(gv, 2)                                  # the database already holds entries
    with pytest.raises(capi.SvoError):
        capi.LoopDetector(ctx, SIZE[0], SIZE[1], 3, max_db_results=100)   # rejected, not silently clamped
    for x in (a, b, c, d_):
        x.close()
    own.close()


def test_a_batch_of_frames_gives_the_verdicts_of_frame_by_frame_submission(ctx, loop_setup):
    """svo_lc_submit_batch: features of 16 images from one set of launches, every stage of their scoring one launch for the
    group -- candidates, scores, normalisation score, status and match of every frame equal those of svo_lc_submit frame by
    frame, bit for bit; host images and device images; a last group that is not full."""
    import torch

    poses, imgs, feats, gv, ov = loop_setup
    own = capi.Context(0)
    a = capi.LoopDetector(ctx, SIZE[0], SIZE[1], 3, seed=5)
    b = capi.LoopDetector(own, SIZE[0], SIZE[1], 3, seed=5)
    c = capi.LoopDetector(own, SIZE[0], SIZE[1], 3, seed=5, dislocal=5, max_entries=200)     # groups of 5
    for d in (a, b, c):
        d.set_vocabulary(gv, 2)
    ref = []
    for img in imgs:
        a.submit(img)
        ref.append(a.collect_ex())
    b.submit_batch(imgs[:50])                                    # host images: 16 + 16 + 16 + 2
    dev = [torch.from_numpy(im).cuda() for im in imgs[50:]]
    b.submit_batch(dev)                                          # device images
    assert b.pending() == len(imgs)
    n_det = 0
    for r in ref:
        g = b.collect_ex()
        assert g["status"] == r["status"] and g["query"] == r["query"] and g["match"] == r["match"]
        assert np.array_equal(g["cand_id"], r["cand_id"]) and np.array_equal(g["cand_score"], r["cand_score"])
        assert g["ns_factor"] == r["ns_factor"]
        n_det += r["status"] == 0
    assert n_det > 0
    # dislocal 5: groups of five; against its own frame-by-frame twin
    d = capi.LoopDetector(ctx, SIZE[0], SIZE[1], 3, seed=5, dislocal=5, max_entries=200)
    d.set_vocabulary(gv, 2)
    c.submit_batch(imgs[:40])
    for img in imgs[:40]:
        d.submit(img)
        x, y = d.collect_ex(), c.collect_ex()
        assert x["status"] == y["status"] and x["match"] == y["match"] and np.array_equal(x["cand_score"], y["cand_score"])
    with pytest.raises(capi.SvoError):
        c.submit_batch(imgs[:] + imgs[:])                        # more frames than the database has room for
    # the same from FEATURES (what rank 0 of a chunk-sharded run receives): all frames in one call
    e = capi.LoopDetector(own, SIZE[0], SIZE[1], 3, seed=5)
    e.set_vocabulary(gv, 2)
    fn = np.array([len(f[0]) for f in feats], np.int32)
    fxy, fdesc = np.zeros((len(feats), 500, 2), np.float32), np.zeros((len(feats), 500, 8), np.uint32)
    for i, f in enumerate(feats):
        fxy[i, :fn[i]], fdesc[i, :fn[i]] = f[0], f[4]
    e.submit_features_batch(fn, fxy, fdesc)
    for r in ref:
        g = e.collect_ex()
        assert g["status"] == r["status"] and g["match"] == r["match"] and np.array_equal(g["cand_score"], r["cand_score"])
    e.close()
    # ... and from arrays with MORE slots per frame than the detector's feature budget (cap 520 > 500: the pinned ring packs them)
    e = capi.LoopDetector(own, SIZE[0], SIZE[1], 3, seed=5)
    e.set_vocabulary(gv, 2)
    wxy, wdesc = np.full((len(feats), 520, 2), 7.0, np.float32), np.full((len(feats), 520, 8), 0xdeadbeef, np.uint32)
    wxy[:, :500], wdesc[:, :500] = fxy, fdesc
    for i in range(len(feats)):
        wxy[i, fn[i]:], wdesc[i, fn[i]:] = 7.0, 0xdeadbeef      # junk beyond every frame's count: must not be read
    e.submit_features_batch(fn, wxy, wdesc)
    got = e.collect_batch(len(ref))
    assert [(v["status"], v["match"]) for v in got] == [(r["status"], r["match"]) for r in ref]
    e.close()
    for x in (a, b, c, d):
        x.close()
    own.close()


def test_detector_sharded_over_ranks_gives_the_one_detector_verdicts(ctx, loop_setup):
    """chunked.sharded_detect with the library's detector (svo_lc_fill_features_batch + svo_lc_submit_features_batch): three
    'ranks', one after another on this GPU, each with a detector of its own -- the frames before its share enter its database
    without being queries, its share (after 8 warm-up frames) is scored and judged.  Status and match of every frame are those
    of ONE detector over the whole stream (the gloo form of the same flow: tests/test_chunked.py)."""
    from ros_stereo_slam_amd import chunked

    poses, imgs, feats, gv, ov = loop_setup
    n = len(feats)
    fn = np.array([len(f[0]) for f in feats], np.int32)
    fxy, fdesc = np.zeros((n, 500, 2), np.float32), np.zeros((n, 500, 8), np.uint32)
    for i, f in enumerate(feats):
        fxy[i, :fn[i]], fdesc[i, :fn[i]] = f[0], f[4]
    one = capi.LoopDetector(ctx, SIZE[0], SIZE[1], 3, seed=5)
    one.set_vocabulary(gv, 2)
    one.submit_features_batch(fn, fxy, fdesc)
    want = [one.collect() for _ in range(n)]
    one.close()
    assert any(v["status"] == 0 for v in want)
    got = []
    for first, end in chunked.detect_shares(n, 3):
        own = capi.Context(0)
        det = capi.LoopDetector(own, SIZE[0], SIZE[1], 3, seed=5)
        det.set_vocabulary(gv, 2)
        # (svo_lc_collect_batch on the second 'rank': the verdicts of k svo_lc_collect calls in one)
        got += chunked.sharded_detect(lambda a, b: det.fill_features_batch(fn[a:b], fxy[a:b], fdesc[a:b]),
                                      lambda a, b: det.submit_features_batch(fn[a:b], fxy[a:b], fdesc[a:b]), det.collect, first, end,
                                      collect_many=det.collect_batch if first > 0 and end < n else None)
        with pytest.raises(capi.SvoError):
            det.collect_batch(1)                    # nothing is queued
        with pytest.raises(capi.SvoError):          # entries are collected in order: no filling while frames are queued
            det.submit_features_batch(fn[:1], fxy[:1], fdesc[:1])
            det.fill_features_batch(fn[:1], fxy[:1], fdesc[:1])
        det.close()
        own.close()
    assert [(v["status"], v["query"], v["match"]) for v in got] == [(v["status"], v["query"], v["match"]) for v in want]


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("k", [3, 9])
def test_detector_sharded_over_ranks_at_larger_k(ctx, loop_setup, k, world):
    """The same rank-after-rank flow at k 3 and k 9 (alpha 0.01: the window is tens of entries long where the shares begin):
    sharded_detect is told the detector's parameters and warms the window up for k * max_distance_between_queries frames --
    with its fixed 8 the first frame of every later share waited for the window at k 9 (tests/test_loopdet_params.py)."""
    from ros_stereo_slam_amd import chunked

    poses, imgs, feats, gv, ov = loop_setup
    n = len(feats)
    fn = np.array([len(f[0]) for f in feats], np.int32)
    fxy, fdesc = np.zeros((n, 500, 2), np.float32), np.zeros((n, 500, 8), np.uint32)
    for i, f in enumerate(feats):
        fxy[i, :fn[i]], fdesc[i, :fn[i]] = f[0], f[4]
    one = capi.LoopDetector(ctx, SIZE[0], SIZE[1], 3, seed=5, alpha=0.01, k=k)
    one.set_vocabulary(gv, 2)
    one.submit_features_batch(fn, fxy, fdesc)
    want = [one.collect() for _ in range(n)]
    one.close()
    shares = chunked.detect_shares(n, world)
    assert all(want[first]["status"] in (0, 7) for first, _ in shares[1:])     # the window is past k where a share begins
    got = []
    for first, end in shares:
        det = capi.LoopDetector(ctx, SIZE[0], SIZE[1], 3, seed=5, alpha=0.01, k=k)
        det.set_vocabulary(gv, 2)
        got += chunked.sharded_detect(lambda a, b: det.fill_features_batch(fn[a:b], fxy[a:b], fdesc[a:b]),
                                      lambda a, b: det.submit_features_batch(fn[a:b], fxy[a:b], fdesc[a:b]), det.collect, first, end,
                                      params=det.prm)
        det.close()
    assert [(v["status"], v["query"], v["match"]) for v in got] == [(v["status"], v["query"], v["match"]) for v in want]


def test_more_than_8192_entries_and_the_wide_candidate_selection(ctx, loop_setup):
    """The candidate selection keeps 8 entries per thread up to 8192 database entries and 16 beyond (eight ranks' shares of the
    driver's bench run are 12 801 frames).  (a) The wide form on the small stream (SVO_BOW_TOPK_PER=16 in a child process) gives
    the narrow form's candidates, scores and verdicts; (b) 8 400 entries -- the stream's features over and over -- run through,
    and a late query's best candidates are earlier copies of the very same frame (score 1)."""
    import json
    import os
    import subprocess
    import sys

    poses, imgs, feats, gv, ov = loop_setup
    n = len(feats)
    fn = np.array([len(f[0]) for f in feats], np.int32)
    fxy, fdesc = np.zeros((n, 500, 2), np.float32), np.zeros((n, 500, 8), np.uint32)
    for i, f in enumerate(feats):
        fxy[i, :fn[i]], fdesc[i, :fn[i]] = f[0], f[4]
    one = capi.LoopDetector(ctx, SIZE[0], SIZE[1], 3, seed=5)
    one.set_vocabulary(gv, 2)
    one.submit_features_batch(fn, fxy, fdesc)
    want = [one.collect_ex() for _ in range(n)]
    one.close()
    # (a) a child process with the wide form forced
    a = gv.arrays()
    np.savez("/tmp/svo_wide_topk.npz", fn=fn, fxy=fxy, fdesc=fdesc, parent=a["parent"], desc=a["desc"], weight=a["weight"], k=gv.k, L=gv.L)
    code = """
import json, numpy as np, torch
torch.cuda.is_available()
from ros_stereo_slam_amd import capi
d = np.load('/tmp/svo_wide_topk.npz')
c = capi.Context(0)
v = capi.Vocabulary.from_arrays(c, int(d['k']), int(d['L']), d['parent'], d['desc'], d['weight'])
det = capi.LoopDetector(c, %d, %d, 3, seed=5)
det.set_vocabulary(v, 2)
det.submit_features_batch(d['fn'], d['fxy'], d['fdesc'])
out = [det.collect_ex() for _ in range(len(d['fn']))]
print(json.dumps([[r['status'], r['match'], r['cand_id'].tolist(), [float(x).hex() for x in r['cand_score']]] for r in out]))
""" % SIZE
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, cwd=root,
                       env=dict(os.environ, SVO_BOW_TOPK_PER="16"))
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    for g, w in zip(got, want):
        assert g[0] == w["status"] and g[1] == w["match"] and g[2] == w["cand_id"].tolist()
        assert g[3] == [float(x).hex() for x in w["cand_score"]]
    # (b) past 8192 entries
    reps = 8400 // n + 1
    big = capi.LoopDetector(ctx, SIZE[0], SIZE[1], 3, seed=5, max_entries=reps * n + 8)
    big.set_vocabulary(gv, 2)
    for _ in range(reps):
        big.submit_features_batch(fn, fxy, fdesc)
    last = None
    for _ in range(reps * n):
        last = big.collect_ex()
    assert last["query"] == reps * n - 1 >= 8400
    assert len(last["cand_id"]) > 0 and abs(last["cand_score"][0] - 1.0) < 1e-9     # an earlier copy of the same frame
    assert all((last["query"] - c) % n == 0 for c in last["cand_id"][:reps - 2])
    big.close()
