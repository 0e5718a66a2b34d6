"""One rendered loop and a table of detector settings, each named for the decision it must change (tests/test_loopdet_params.py
proves on the CPU, from the oracle alone, that it does; tests/test_gpu_loopdet_params.py compares the library with the oracle at
every one of them).  The stream is the one tests/test_gpu_bow.py uses: 134 frames of 480 x 160 around a rounded rectangle that
comes back to its start at frame 114, features in cv::ORB's shape, a k 9 / L 6 vocabulary trained on every second frame."""
import contextlib
import functools

import numpy as np

from oracle import orc
from oracle.loop_detector import LoopDetector, Params

SIZE, K4, N_FRAMES, N_FEATURES = (480, 160), (270.0, 270.0, 240.0, 80.0), 134, 500
VOC_K, VOC_L, VOC_SEED, SEED = 9, 6, 20261003, 5
STATUS = ("LOOP_DETECTED", "CLOSE_MATCHES_ONLY", "NO_DB_RESULTS", "LOW_NSS_FACTOR", "LOW_SCORES", "NO_GROUPS",
          "NO_TEMPORAL_CONSISTENCY", "NO_GEOMETRICAL_CONSISTENCY")
DET, CLOSE, NO_DB, LOW_NSS, LOW_SC, NO_GRP, NO_TEMP, NO_GEOM = range(8)


def loop_images(n=N_FRAMES):
    """the left views of test_gpu_bow._loop_images (the right ones are never looked at: not rendered)"""
    from ros_stereo_slam_amd import synth

    poses = synth.loop_trajectory(n, half_x=6, half_z=10, radius=4, step=0.5)
    sc = synth.Scene(wall_x=14, z_min=-18, z_max=18)
    return [sc.render(R, t, K=K4, size=SIZE)[0] for R, t in poses]


@functools.lru_cache(maxsize=1)
def stream():
    """-> (images, [(xy, desc)] from the oracle's extractor, the oracle's vocabulary); made once per process"""
    orc.load()
    imgs = loop_images()
    feats = []
    for im in imgs:
        f = orc.orb_extract_cv(im, N_FEATURES, 20, 8, 1.2, None)
        feats.append((f[0], f[5]))
    voc = orc.Vocabulary.train([d for _, d in feats[::2]], k=VOC_K, L=VOC_L, seed=VOC_SEED)
    return imgs, feats, voc


def pack(feats, cap=N_FEATURES):
    """[(xy, desc)] -> the arrays of svo_lc_submit_features_batch: n [F], xy [F, cap, 2], desc [F, cap, 8]"""
    fn = np.array([len(xy) for xy, _ in feats], np.int32)
    fxy, fdesc = np.zeros((len(feats), cap, 2), np.float32), np.zeros((len(feats), cap, 8), np.uint32)
    for i, (xy, desc) in enumerate(feats):
        fxy[i, :fn[i]], fdesc[i, :fn[i]] = xy, desc
    return fn, fxy, fdesc


def f32(x):
    """svo_lc_params keeps alpha and min_nss_factor as floats, as the reference's Parameters do (float alpha, float
    min_nss_factor; the comparison is made in double): the oracle is given the value the field holds"""
    return float(np.float32(x))


class Entry:
    """``params``: what is moved off the reference's defaults; ``voc`` / ``di_levels``: the scoring mode; ``reaches``:
    statuses that must occur; ``branch``: a predicate over (this run, the default run, the runs by name) for what the entry is
    named for when a status alone does not show it; ``unlike``: further entries (beside the defaults) whose verdicts it must
    differ from -- the sibling that differs in the named parameter alone."""

    def __init__(self, name, params=None, voc=True, di_levels=2, reaches=(), branch=None, unlike=()):
        self.name, self.params, self.voc, self.di_levels = name, dict(params or {}), voc, di_levels
        self.reaches, self.branch, self.unlike = tuple(reaches), branch, tuple(unlike)

    def __repr__(self):
        return self.name

    def lib_params(self):
        """keyword arguments of capi.LoopDetector"""
        return dict(self.params, seed=SEED)

    def oracle_params(self):
        p = dict(self.params, seed=SEED)
        for k in ("alpha", "min_nss_factor"):
            p[k] = f32(p.get(k, getattr(Params(), k)))
        return Params(**p)


class Recorder(LoopDetector):
    """The oracle's detector, its computations untouched, noting per frame what its verdict went through: the islands it
    formed, the window's length after the update, whether the geometric check ran."""

    def detect_features(self, xy, desc):
        self.note = dict(n_islands=None, islands=None, window=None, geom=None)
        res = super().detect_features(xy, desc)
        ids, sc, ns = self.last_query
        return dict(res, cand_id=list(ids), cand_score=list(sc), ns=ns, **self.note)

    def _islands(self, q):
        out = super()._islands(q)
        self.note["n_islands"], self.note["islands"] = len(out), [(t["first"], t["last"]) for t in out]
        return out

    def _update_window(self, island, entry_id):
        super()._update_window(island, entry_id)
        self.note["window"] = self.window["nentries"]

    def _geometric(self, old_entry, xy, desc, node=None):
        ok = super()._geometric(old_entry, xy, desc, node)
        self.note["geom"] = bool(ok)
        return ok


@contextlib.contextmanager
def memoised_bow_query():
    """orc.bow_query is a pure function of its five arrays and takes nine tenths of a detector run; the table runs it with the
    same arrays at every setting.  An exact memo on the bytes of ALL its inputs, in place for the length of a run."""
    plain = orc.bow_query

    def cached(qw, qv, db_w, db_v, db_n):
        key = tuple(np.ascontiguousarray(a).tobytes() for a in (qw, qv, db_w, db_v, db_n)) + (np.shape(db_w),)
        if key not in _MEMO:
            _MEMO[key] = plain(qw, qv, db_w, db_v, db_n)
        return _MEMO[key]

    orc.bow_query = cached
    try:
        yield
    finally:
        orc.bow_query = plain


_MEMO = {}
_RUNS = {}


def run_oracle(entry, fill=0, feats=None, voc=None):
    """The oracle over the stream at ``entry``'s setting: the first ``fill`` frames enter its database without being queries.
    -> one record per queried frame: status, query, match, cand_id, cand_score, ns and the Recorder's notes."""
    own = feats is None
    if own:
        if (entry.name, fill) in _RUNS:
            return _RUNS[entry.name, fill]
        _, feats, voc = stream()
    det = Recorder(entry.oracle_params(), voc=voc if entry.voc else None, di_levels=entry.di_levels)
    with memoised_bow_query():
        for xy, desc in feats[:fill]:
            det.fill(xy, desc)
        out = [det.detect_features(xy, desc) for xy, desc in feats[fill:]]
    if own:
        _RUNS[entry.name, fill] = out
    return out


def verdicts(run):
    return [(r["status"], r["match"]) for r in run]


def statuses(run):
    return {r["status"] for r in run}


# ---- the branches that a status alone does not show -------------------------------------------------------------------------
def _islands_against(sibling, more):
    """islands split / merged: some frame forms more / fewer islands than the same frame of the sibling run"""
    def check(run, default, runs):
        pairs = [(a["n_islands"], b["n_islands"]) for a, b in zip(run, runs[sibling]) if None not in (a["n_islands"], b["n_islands"])]
        return any(a > b for a, b in pairs) if more else any(a < b for a, b in pairs)
    return check


def _window_restarts_where_sibling_grows(sibling):
    def check(run, default, runs):
        return any(a["window"] == 1 and b["window"] is not None and b["window"] > 1 for a, b in zip(run, runs[sibling]))
    return check


def _window_grows_where_sibling_restarts(sibling):
    def check(run, default, runs):
        return any(a["window"] is not None and a["window"] > 1 and b["window"] == 1 for a, b in zip(run, runs[sibling]))
    return check


def _window_longer_than(n):
    def check(run, default, runs):
        return max((r["window"] or 0) for r in run) > n
    return check


def _detects_where_sibling_fails(sibling):
    def check(run, default, runs):
        return any(a["status"] == DET and b["status"] == NO_GEOM for a, b in zip(run, runs[sibling]))
    return check


def _fails_where_sibling_detects(sibling):
    def check(run, default, runs):
        return any(a["status"] == NO_GEOM and b["status"] == DET for a, b in zip(run, runs[sibling]))
    return check


def _fewer_candidates(run, default, runs):
    return max(len(r["cand_id"]) for r in run) == 1 < max(len(r["cand_id"]) for r in default)


def _first_query_at(frame):
    def check(run, default, runs):
        return run[frame - 1]["status"] == CLOSE and run[frame]["status"] != CLOSE
    return check


# ---- the table ---------------------------------------------------------------------------------------------------------------
# At the reference's defaults this stream is an easy one: 21 frames CLOSE_MATCHES_ONLY, 94 LOW_SCORES (the best candidate
# scores 0.01 against a normalisation score of 0.15), NO_TEMPORAL_CONSISTENCY at frame 115 and LOOP_DETECTED from 116 on, every
# one with one island and far more matches than min_Fpoints.  A parameter of the islands, the window or the geometric check
# that cannot act there is paired with an alpha low enough that the unrelated frames along the way reach those stages too:
LOOSE = dict(alpha=0.05)     # observed: 81 frames change verdict; up to 13 islands a frame; 37 detections, 33 / 29 frames fail the window / the geometry
SPARSE = dict(alpha=0.125)   # observed: 26 frames change; the frames that reach the window lie 2 to 14 frames apart before the loop closes
DEFAULT = Entry("defaults", {}, reaches=(DET, CLOSE, LOW_SC, NO_TEMP))

TABLE = [
    # alpha (removeLowScores) and the siblings of the paired entries below
    Entry("alpha_loose_lets_unrelated_frames_through", LOOSE, reaches=(DET, LOW_SC, NO_TEMP, NO_GEOM)),
    Entry("alpha_sparse_leaves_gaps_between_window_updates", SPARSE, reaches=(DET, LOW_SC, NO_TEMP)),
    # observed: frames 116 and 128, detections at the defaults, end in LOW_SCORES; 16 frames still detect
    Entry("alpha_one_cuts_some_loop_frames_to_low_scores", dict(alpha=1.0), reaches=(LOW_SC, DET),
          branch=lambda run, default, runs: any(a["status"] == LOW_SC and b["status"] == DET for a, b in zip(run, default))),
    # k: more than k consistent matches.  Observed alone: frame 115 detects at k 0; 116 / 116-117 wait at k 2 / 3
    Entry("k0_no_frame_waits_for_the_window", dict(k=0),
          branch=lambda run, default, runs: NO_TEMP not in statuses(run) and NO_TEMP in statuses(default)),
    Entry("k2_one_more_frame_waits", dict(k=2), reaches=(NO_TEMP, DET)),
    Entry("k3_two_more_frames_wait", dict(k=3), reaches=(NO_TEMP, DET)),
    # observed: 61 frames NO_TEMPORAL_CONSISTENCY against 33 at k 1
    Entry("k3_loose_short_chains_never_pass", dict(LOOSE, k=3), reaches=(NO_TEMP, DET, NO_GEOM), unlike=("alpha_loose_lets_unrelated_frames_through",)),
    # the normalisation.  Observed: without it alpha 0.9 is an absolute cut no score reaches: every query LOW_SCORES
    Entry("nss_off_alpha_is_absolute", dict(use_nss=0), reaches=(LOW_SC,),
          branch=lambda run, default, runs: statuses(run) == {CLOSE, LOW_SC} and all(r["ns"] == 1.0 for r in run if r["cand_id"])),
    # observed: an absolute cut of 0.01: 34 detections, 35 / 22 frames fail the window / the geometry
    Entry("nss_off_small_absolute_alpha", dict(use_nss=0, alpha=0.01), reaches=(DET, LOW_SC, NO_TEMP, NO_GEOM)),
    # observed: normalisation scores run from 0.08 to 0.21; 16 frames fall below 0.125, one still detects
    Entry("min_nss_factor_stops_weakly_normalised_frames", dict(min_nss_factor=0.125), reaches=(LOW_NSS, LOW_SC, DET)),
    # islands: min_matches_per_group is a LENGTH in entry ids, and a single candidate is an island whatever its length
    Entry("min_matches_2_drops_single_entry_islands", dict(LOOSE, min_matches_per_group=2), reaches=(NO_GRP, DET),
          unlike=("alpha_loose_lets_unrelated_frames_through",)),             # observed: 15 frames NO_GROUPS
    Entry("min_matches_3_drops_short_islands", dict(min_matches_per_group=3), reaches=(NO_GRP, DET)),   # observed: 6 frames, alone
    Entry("intragroup_gap_1_splits_islands", dict(LOOSE, max_intragroup_gap=1), branch=_islands_against("alpha_loose_lets_unrelated_frames_through", more=True),
          unlike=("alpha_loose_lets_unrelated_frames_through",)),             # observed: up to 50 islands a frame (13)
    Entry("intragroup_gap_6_merges_islands", dict(LOOSE, max_intragroup_gap=6), branch=_islands_against("alpha_loose_lets_unrelated_frames_through", more=False),
          unlike=("alpha_loose_lets_unrelated_frames_through",)),             # observed: at most 9 islands a frame (13)
    # the temporal window
    Entry("group_distance_0_restarts_the_window", dict(max_distance_between_groups=0), reaches=(NO_TEMP, DET),
          branch=_window_restarts_where_sibling_grows("defaults")),                       # observed alone: frames 121 123 127 131 133
    Entry("query_distance_1_restarts_the_window", dict(SPARSE, max_distance_between_queries=1),
          branch=_window_restarts_where_sibling_grows("alpha_sparse_leaves_gaps_between_window_updates"), unlike=("alpha_sparse_leaves_gaps_between_window_updates",)),   # observed: 49, 83
    Entry("query_distance_5_carries_the_window_over", dict(SPARSE, max_distance_between_queries=5),
          branch=_window_grows_where_sibling_restarts("alpha_sparse_leaves_gaps_between_window_updates"),
          unlike=("alpha_sparse_leaves_gaps_between_window_updates",)),       # observed: frames 53 and 61
    # the geometric check (direct index, neighbour ratio, F-matrix RANSAC).  Observed on LOOSE: 37 detections / 29 failures
    Entry("min_fpoints_8_accepts_thin_matches", dict(LOOSE, min_Fpoints=8), reaches=(DET,),
          branch=_detects_where_sibling_fails("alpha_loose_lets_unrelated_frames_through"),
          unlike=("alpha_loose_lets_unrelated_frames_through",)),             # observed: 66 detections, no failure left
    Entry("min_fpoints_14_sibling_of_the_ransac_probability", dict(LOOSE, min_Fpoints=14), reaches=(DET, NO_GEOM),
          unlike=("alpha_loose_lets_unrelated_frames_through",)),
    Entry("min_fpoints_100_refuses_ordinary_matches", dict(LOOSE, min_Fpoints=100), reaches=(DET, NO_GEOM),
          branch=_fails_where_sibling_detects("alpha_loose_lets_unrelated_frames_through"),
          unlike=("alpha_loose_lets_unrelated_frames_through",)),             # observed: 20 detections / 46 failures
    Entry("neighbour_ratio_04_keeps_fewer_pairs", dict(LOOSE, max_neighbor_ratio=0.4), reaches=(DET, NO_GEOM),
          branch=_fails_where_sibling_detects("alpha_loose_lets_unrelated_frames_through"),
          unlike=("alpha_loose_lets_unrelated_frames_through",)),             # observed: 36 / 30
    Entry("neighbour_ratio_09_keeps_more_pairs", dict(LOOSE, max_neighbor_ratio=0.9), reaches=(DET, NO_GEOM),
          branch=_detects_where_sibling_fails("alpha_loose_lets_unrelated_frames_through"),
          unlike=("alpha_loose_lets_unrelated_frames_through",)),             # observed: 45 / 21
    Entry("reprojection_error_05_counts_fewer_inliers", dict(LOOSE, max_reprojection_error=0.5), reaches=(DET, NO_GEOM),
          branch=_fails_where_sibling_detects("alpha_loose_lets_unrelated_frames_through"),
          unlike=("alpha_loose_lets_unrelated_frames_through",)),             # observed: 26 / 40
    Entry("reprojection_error_4_counts_more_inliers", dict(LOOSE, max_reprojection_error=4.0), reaches=(DET, NO_GEOM),
          branch=_detects_where_sibling_fails("alpha_loose_lets_unrelated_frames_through"),
          unlike=("alpha_loose_lets_unrelated_frames_through",)),             # observed: 57 / 9
    Entry("one_ransac_iteration_misses_models", dict(LOOSE, max_ransac_iterations=1), reaches=(DET, NO_GEOM),
          branch=_fails_where_sibling_detects("alpha_loose_lets_unrelated_frames_through"),
          unlike=("alpha_loose_lets_unrelated_frames_through",)),             # observed: 24 / 42
    # ransac_probability only shortens a RANSAC that has a model already: it acts where an early model falls just short of
    # min_Fpoints and a later one would not.  Observed: nowhere at min_Fpoints 8 - 13; at 14, frame 28 (a grid over min_Fpoints
    # 9 .. 28, reprojection errors 0.5 / 1 / 2 and ratios 0.6 / 0.8 / 0.9 found three such settings, this the plainest)
    Entry("ransac_probability_05_stops_before_the_better_model", dict(LOOSE, min_Fpoints=14, ransac_probability=0.5),
          branch=_fails_where_sibling_detects("min_fpoints_14_sibling_of_the_ransac_probability"),
          unlike=("min_fpoints_14_sibling_of_the_ransac_probability",)),
    # the database query
    Entry("one_db_result_one_island", dict(LOOSE, max_db_results=1), branch=_fewer_candidates,
          unlike=("alpha_loose_lets_unrelated_frames_through",)),             # observed: 48 / 15 frames fail the window / the geometry
    # observed: frame 2 is the first query and finds no entry with a common word (NO_DB_RESULTS); frames 3 .. 20 LOW_SCORES
    Entry("dislocal_1_queries_from_frame_2", dict(dislocal=1), reaches=(NO_DB, LOW_SC, DET), branch=_first_query_at(2)),
    # the edge of "a group of 16 frames cannot hold its own candidates": groups of 16 with candidates 16 entries back
    Entry("dislocal_16_queries_from_frame_17", dict(dislocal=16), reaches=(LOW_SC, DET), branch=_first_query_at(17)),
    # the direct index: pairs are sought under a common node di_levels above the leaves -- 0: the same word, 3: a 729th of the tree
    Entry("di_levels_0_same_word_only", dict(LOOSE), di_levels=0, reaches=(DET, NO_GEOM),
          branch=_fails_where_sibling_detects("alpha_loose_lets_unrelated_frames_through"),
          unlike=("alpha_loose_lets_unrelated_frames_through",)),             # observed: 26 / 40
    Entry("di_levels_1", dict(LOOSE), di_levels=1, reaches=(DET, NO_GEOM),
          branch=_fails_where_sibling_detects("alpha_loose_lets_unrelated_frames_through"),
          unlike=("alpha_loose_lets_unrelated_frames_through",)),             # observed: 26 / 40
    Entry("di_levels_3_wide_nodes", dict(LOOSE), di_levels=3, reaches=(DET, NO_GEOM),
          branch=_detects_where_sibling_fails("alpha_loose_lets_unrelated_frames_through"),
          unlike=("alpha_loose_lets_unrelated_frames_through",)),             # observed: 64 / 2
    # without a vocabulary: the share of query descriptors with a neighbour within hamming_threshold bits
    # observed at 32: unrelated frames share next to nothing (92 frames LOW_SCORES, 20 detections)
    Entry("hamming_32_unrelated_frames_score_low", dict(hamming_threshold=32), voc=False, reaches=(DET, LOW_SC),
          unlike=("hamming_96_every_frame_resembles_every_other",)),
    # observed at 96: every frame passes the cut, 86 fail the exhaustive geometric check, the window grows to 97
    Entry("hamming_96_every_frame_resembles_every_other", dict(hamming_threshold=96), voc=False, reaches=(DET, NO_GEOM),
          branch=_window_longer_than(50), unlike=("hamming_32_unrelated_frames_score_low",)),
]
BY_NAME = {e.name: e for e in [DEFAULT] + TABLE}

# what the sharded run is checked at (tests/test_loopdet_params.py, test_chunked.py, test_gpu_bow.py): with an alpha of 0.01 nearly
# every frame passes the cut and the window is 20 to 47 entries long where the shares of 2 and 3 ranks begin (frames 67; 45, 90)
SHARDED = {k: Entry(f"sharded_k{k}", dict(alpha=0.01, k=k)) for k in (3, 9)}
