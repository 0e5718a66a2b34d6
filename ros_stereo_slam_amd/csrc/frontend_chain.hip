// frontend_chain.hip -- the chain runner of the stereo-VO front-end: svo_vo_run_chunk, svo_vo_run_chunks.
//
// A run of consecutive frames WITHOUT the host in the loop (the "chunk runner" of SURVEY.md 8b/8e): the host queues the
// launches of every frame and waits ONCE, when all of them are queued.  The per-frame decisions of the reference's
// host policy are taken by pnp_finish_kernel on the device (VoChain, svo_internal.h):
//   keyframe iff fewer than keyframe_min_inliers PnP inliers    src/VisualSLAM.cpp:120
//   no keyframe: the tracked sets become the reference sets    src/VisualSLAM.cpp:143-146 (a copy inside pnp_finish)
//   keyframe: insertKeyFrames at the refined pose               src/keyFrameManagement.cpp:9-31
// The keyframe path (LK left -> right, ANMS, status filter, F-RANSAC, DLT triangulation) is queued for EVERY frame; its
// kernels leave at once unless the device flag says keyframe.  The rare slow paths stop the chain (every later kernel
// of the chunk leaves at once) and come back to the host: fewer than 10 inliers at 1 px -- the 8 px retry of
// src/keyFrameManagement.cpp:85-92 -- and a reference set of fewer than 5 points.  The host handles the frame with the
// frame-by-frame code and queues the rest of the chunk again.
//
// Results: exactly those of n_frames calls of svo_vo_track(..., force_keyframe = 0) -- every stage sees the same
// inputs and seeds (tests/test_gpu_frontend.py::test_run_chunk_*).
//
// pipeline (one chunk, device images): four HIP streams, see svo_vo and chain_enqueue_pipelined.  The PnP of frame t runs on a
// stream of its own while the context's stream builds the pyramids of frame t+1 and tracks into them from the points
// frame t kept -- which is what frame t+1 does unless frame t turns out to be a keyframe, in which case a second tracking
// launch (gated on the keyframe flag) redoes it from the new keyframe's points; the stereo path of every frame runs a
// frame ahead on a third stream.
#include <chrono>
#include <string>
#include <thread>
#include <vector>

#include "frontend_state.hip.h"

namespace {

// debug (SVO_CHAIN_STAMPS): the constant 100 MHz clock, written by a one-lane launch between the stages of a stream
__global__ void stamp_kernel(unsigned long long *dst) { *dst = wall_clock64(); }

}  // namespace

struct ChainRun {            // one chunk of a lock-step set
    svo_vo *v;
    const uint8_t *const *lefts, *const *rights;
    int n_frames, mem;
    // results (caller's arrays, any may be null except R_out / t_out)
    double *R_out, *t_out;
    int *inliers_out, *tracked_out;
    uint8_t *keyframe_out;
    int n_done = 0, rc = SVO_OK;
    // working state
    int frame0 = 0;                                  // v->frame when the run was queued
    svo_pyramid *p0 = nullptr, *p1 = nullptr, *p2 = nullptr;  // pyramid roles when the run was queued: ref, cur, next
    VoChain end;                                     // the chain state after the run
    int halt_set = 0;                                // which tracked set the frame that halted the chain wrote
};

static ChainRun make_run(svo_vo *v, const uint8_t *const *lefts, const uint8_t *const *rights, int n_frames, int mem,
                         double *R_out, double *t_out, int *inliers_out, int *tracked_out, uint8_t *keyframe_out)
{
    return ChainRun{v, lefts, rights, n_frames, mem, R_out, t_out, inliers_out, tracked_out, keyframe_out};
}

static int chain_prepare(ChainRun &r)
{
    svo_vo *v = r.v;
    if (r.n_frames > v->out_cap) {
        if (v->h_out)
            (void)hipHostFree(v->h_out);
        v->h_out = nullptr;
        v->out_cap = 0;
        // grown in big steps: pinning memory takes a fraction of a millisecond and synchronises with the device
        // (a run of 50 frames after a warm-up of 20 re-pinned all 64 front-ends' buffers inside the benchmark's clock)
        const int cap = r.n_frames < 1024 ? 1024 : 2 * r.n_frames;
        SVO_HIP(hipHostMalloc(reinterpret_cast<void **>(&v->h_out), sizeof(VoOut) * (size_t)cap, hipHostMallocDefault));
        v->out_cap = cap;
    }
    VoChain *c = v->h_chain;
    memset(c, 0, sizeof(*c));
    static const bool dry = getenv("SVO_CHAIN_DRY") != nullptr;  // experiment: every kernel leaves at once -> the host's own cost
    c->run = dry ? 0 : 1;
    c->kf = 0;
    c->nref = v->nref;
    c->frame = 0;
    c->halt_code = SVO_HALT_NONE;
    c->kf_n = v->kf_n;
    memcpy(c->R, v->R, sizeof(c->R));
    memcpy(c->t, v->t, sizeof(c->t));
    c->kf_min = v->prm.keyframe_min_inliers;
    c->retry_below = v->prm.pnp_retry_below;  // src/keyFrameManagement.cpp:85
    c->ref2d = v->ref2d;
    c->ref3d = v->ref3d;
    c->out = v->h_out;
    // the previous run's wait has long returned: the pinned staging copy is free again
    SVO_HIP(hipMemcpyAsync(v->d_chain, c, sizeof(VoChain), hipMemcpyHostToDevice, v->ctx->stream));
    r.frame0 = v->frame;
    r.p0 = v->pyr_ref;
    r.p1 = v->pyr_cur;
    r.p2 = v->pyr_next;
    r.n_done = 0;
    r.rc = SVO_OK;
    return SVO_OK;
}

// queue the tracking pass ref -> cur of k chunks as one launch
static int chain_lk(svo_ctx *ctx, int k, svo_vo *const *vs, svo_pyramid *const *prev, svo_pyramid *const *next,
                    const float *const *pts, const int *const *d_n, const int *const *gates)
{
    LkJob lk[SVO_LK_MAX_JOBS];
    for (int a = 0; a < k; a++)
        lk[a] = lk_job(prev[a], next[a], pts[a], vs[a]->cap, d_n[a], vs[a]->a2, vs[a]->status, nullptr, gates[a]);
    return svo_launch_lk_batch(ctx, k, lk, prev[0]);
}

// status filter (src/tracking.cpp:54-64), F-RANSAC at 1 px + its mask filter (:75-88): the tracked sets and their count
// set: which of the two tracked sets / count slots the frame writes (pipelined chunks alternate)
// st_par: which of the two status-byte buffers the frame's tracking passes wrote (pipelined chunk).
// kf_slot >= 0 (pipelined chunk, one front-end): the 2-D half only -- the 3-D column follows on the PnP stream,
// chain_filters_3d -- and, when the previous frame was a keyframe (the device flag), from the sets of the tracking pass
// that started at its points: reference points = hand-over set kf_slot, tracked points / status bytes = a2k / statusk [kbuf].
static int chain_filters(svo_ctx *ctx, int k, svo_vo *const *vs, int set = 0, int kf_slot = -1, int st_par = 0, int kbuf = 0)
{
    svo_compact_job c1[SVO_LK_MAX_JOBS], c2[SVO_LK_MAX_JOBS];
    svo_fransac_job fj[SVO_LK_MAX_JOBS];
    for (int a = 0; a < k; a++) {
        svo_vo *v = vs[a];
        const TrackedSet ts = tracked_set(v, set);
        int *cnt_st = v->d_cnt + CNT_STATUS;
        const int *run = &v->d_chain->run;
        if (kf_slot >= 0) {
            c1[a] = {st_par ? v->status_b : v->status, v->cap, &v->d_chain->nref, {v->ref2d, v->a2, nullptr},
                     {v->b2, v->c2, nullptr}, {2, 2, 0}, cnt_st, run};
            c1[a].alt_sel = &v->d_chain->kf;
            c1[a].alt_mask = v->statusk[kbuf];
            c1[a].alt_in[0] = v->h_x1[kf_slot];
            c1[a].alt_in[1] = v->a2k[kbuf];
            c1[a].alt_d_n = v->h_cnt + kf_slot;
            c2[a] = {v->mask, v->cap, cnt_st, {v->c2, nullptr, nullptr}, {ts.p2, nullptr, nullptr}, {2, 0, 0}, ts.cnt};
        } else {
            c1[a] = {v->status, v->cap, &v->d_chain->nref, {v->ref2d, v->a2, v->ref3d}, {v->b2, v->c2, v->a3}, {2, 2, 3},
                     cnt_st, run};
            c2[a] = {v->mask, v->cap, cnt_st, {v->c2, v->a3, nullptr}, {ts.p2, ts.p3, nullptr}, {2, 3, 0}, ts.cnt};
        }
        // the mask compaction rides with the F-RANSAC
        fj[a] = {v->b2, v->c2, v->cap, cnt_st, v->prm.f_thr_temporal, 0.99, 1000, stage_seed(v, v->frame, 0), v->mask, nullptr,
                 nullptr, nullptr, &c2[a], run};
    }
    int rc;
    if ((rc = svo_launch_compact_batch(ctx, k, c1)) || (rc = svo_launch_fransac_batch(ctx, k, fj)))
        return rc;
    return SVO_OK;
}

// The 3-D column of the two filters above, for a pipelined chunk, on the PnP stream once the frame's status bytes and
// F-RANSAC mask exist: reference points (by then the keyframe's cloud has been placed, if the previous frame was one)
// -> status filter -> mask filter -> the tracked 3-D set the PnP reads.
static int chain_filters_3d(svo_ctx *ctx, svo_vo *v, int set, int st_par, int kbuf)
{
    const int *run = &v->d_chain->run;
    svo_compact_job c[2];
    c[0] = {st_par ? v->status_b : v->status, v->cap, &v->d_chain->nref, {v->ref3d, nullptr, nullptr}, {v->a3, nullptr, nullptr},
            {3, 0, 0}, v->d_cnt + CNT_3D_STATUS, run};
    c[0].alt_sel = &v->d_chain->kf;  // still the previous frame's decision
    c[0].alt_mask = v->statusk[kbuf];
    c[1] = {v->mask, v->cap, v->d_cnt + CNT_3D_STATUS, {v->a3, nullptr, nullptr}, {tracked_set(v, set).p3, nullptr, nullptr},
            {3, 0, 0}, v->d_cnt + CNT_3D_MASK, run};
    int rc;
    if ((rc = svo_launch_compact_batch(ctx, 1, &c[0])) || (rc = svo_launch_compact_batch(ctx, 1, &c[1])))
        return rc;
    return SVO_OK;
}

// the PnP-RANSAC problem of a localisation as the chain runner queues it: solvePnPRansac(100, 1 px, 0.99) over the
// tracked set `set`, the frame's policy decided by the finishing kernel (VoChain)
static svo_pnp_job pnp_job(svo_vo *v, int set)
{
    const TrackedSet ts = tracked_set(v, set);
    svo_pnp_job q;
    q.obj = ts.p3;
    q.img = ts.p2;
    q.cap = v->cap;
    q.d_n = ts.cnt;
    q.K4[0] = v->prm.fx;
    q.K4[1] = v->prm.fy;
    q.K4[2] = v->prm.cx;
    q.K4[3] = v->prm.cy;
    q.iterations = 100;
    q.reproj_err = 1.0;
    q.confidence = 0.99;
    q.seed = stage_seed(v, v->frame, 1);
    q.refine_iters = 20;
    q.inliers = ts.idx;
    q.mask = nullptr;
    q.d_result = ts.rec;
    q.chain = v->d_chain;
    q.cnt_trk = ts.cnt;
    return q;
}

static int chain_pnp(svo_ctx *ctx, int k, svo_vo *const *vs, int set = 0, bool split = false)
{
    svo_pnp_job pj[SVO_LK_MAX_JOBS];
    for (int a = 0; a < k; a++)
        pj[a] = pnp_job(vs[a], set);
    return svo_launch_pnp_ransac_batch(ctx, k, pj, split);
}

// the refinement a split chain_pnp left undone, for the frame if it is a keyframe / if it is none
static int chain_pnp_refine(svo_ctx *ctx, svo_vo *v, int set, bool keyframes)
{
    const svo_pnp_job pj = pnp_job(v, set);
    return svo_launch_pnp_refine(ctx, 1, &pj, keyframes);
}

// the pyramids of one frame of na chunks from device images: the left images and, in the same set of launches, the right
// ones; each chunk's while its chain is live
static int build_pyramids(svo_ctx *ctx, int na, svo_vo *const *va, svo_pyramid *const *lp, svo_pyramid *const *rp,
                          const uint8_t *const *li, const uint8_t *const *ri)
{
    svo_pyramid *pyrs[2 * SVO_LK_MAX_JOBS];
    const uint8_t *imgs[2 * SVO_LK_MAX_JOBS];
    const int *g[2 * SVO_LK_MAX_JOBS];
    for (int a = 0; a < na; a++) {
        pyrs[a] = lp[a];
        imgs[a] = li[a];
        pyrs[na + a] = rp[a];
        imgs[na + a] = ri[a];
        g[a] = g[na + a] = &va[a]->d_chain->run;
    }
    return svo_build_pyramids_from_device(ctx, 2 * na, pyrs, imgs, g);
}

// Device time stamps between the stages of a pipelined chunk (SVO_CHAIN_STAMPS, svo_vo_set_stage_stamps), 8 per frame:
// A0 before filters, A1 after, A2 after the tracking launch, B0 before hypotheses, B1 decided, B2 handed over, C0 / C1
// around the stereo path.
constexpr int kMaxStampFrames = 4096;

// after a stamped run is queued: wait, read, keep (and print, with the environment switch) the mean intervals over the
// middle of the run
static int chain_read_stamps(svo_vo *v, int nf, bool print)
{
    SVO_HIP(hipStreamSynchronize(v->ctx->stream));
    SVO_HIP(hipStreamSynchronize(v->lane.ctx->stream));
    const int n = nf < kMaxStampFrames ? nf : kMaxStampFrames;
    std::vector<unsigned long long> h((size_t)8 * n);
    SVO_HIP(hipMemcpy(h.data(), v->d_stamps, h.size() * sizeof(h[0]), hipMemcpyDeviceToHost));
    auto T = [&](int f, int k) { return (double)h[(size_t)8 * f + k] * 0.01; };  // 100 MHz -> us
    double cyc = 0, filt = 0, lk = 0, a_wait = 0, b_lag = 0, pnp = 0, hand = 0, c_lag = 0, c_len = 0;
    int m = 0;
    for (int f = 20; f + 3 < n; f++, m++) {
        cyc += T(f + 1, 0) - T(f, 0);
        filt += T(f, 1) - T(f, 0);
        lk += T(f, 2) - T(f, 1);
        a_wait += T(f + 1, 0) - T(f, 2);
        b_lag += T(f, 3) - T(f, 1);
        pnp += T(f, 4) - T(f, 3);
        hand += T(f, 5) - T(f, 4);
        c_lag += T(f, 6) - T(f, 2);
        c_len += T(f, 7) - T(f, 6);
    }
    const double vals[SVO_STAGE_COUNT] = {cyc / m, filt / m, lk / m, a_wait / m, b_lag / m, pnp / m, hand / m, c_lag / m, c_len / m};
    for (int i = 0; i < SVO_STAGE_COUNT; i++)
        v->stage_us[i] = vals[i];
    v->stage_frames = m;
    if (print)
        fprintf(stderr, "[svo chain] device us per frame (stamps): cycle %.1f = filters %.1f + tracking launch %.1f + wait for B %.1f | "
                        "B starts %.1f after the filters, PnP to decision %.1f, refine + hand-over of a keyframe %.1f | C starts %.1f "
                        "after the launch, stereo path %.1f\n", cyc / m, filt / m, lk / m, a_wait / m, b_lag / m, pnp / m, hand / m,
                c_lag / m, c_len / m);
    return SVO_OK;
}

// Queue the frames of ONE chunk (device images) on four streams (see svo_vo).  Nothing on A waits for the frame's decision:
// after the filters of frame f it runs BOTH tracking passes into frame f+1 -- from the tracked set and from the 2-D points
// the stereo path of f has left -- as one launch (the launch lasts as long as its slowest keypoint: two passes cost less
// than two launches), and the filters of f+1 take the status bytes and points of the one the decision points to (the
// compaction selects by the keyframe flag on the device).  B: PnP hypotheses, the decision, then a keyframe's
// refinement and the hand-over of its sets (the 2-D points become the reference set, the cloud is placed with
// the refined pose), which A waits for before the next filters; any other frame's refinement after that.
// C: the stereo path of EVERY frame, two frames ahead, started when A's tracking launch has ended (its own
// tracking pass then runs beside A's filters instead of beside A's launch).  D: the pyramids, two frames ahead.
static int chain_enqueue_pipelined(ChainRun &r)
{
    svo_vo *v = r.v;
    svo_ctx *ctx = v->ctx;
    int rc;
    if (r.n_frames == 0)
        return SVO_OK;
    hipStream_t sA = ctx->stream, sB = v->stream_b, sC = v->lane.ctx->stream, sD = v->stream_p;
    hipStream_t sE = sD;  // the keyframe passes share the pyramids' stream: a fifth busy queue costs more than it brings
    const hipEvent_t *ev = v->ev;
    static const bool stamps_env = getenv("SVO_CHAIN_STAMPS") != nullptr;
    const bool stamps = stamps_env || v->stamps_on;
    if (stamps && !v->d_stamps)
        SVO_HIP(hipMalloc(reinterpret_cast<void **>(&v->d_stamps), sizeof(unsigned long long) * 8 * kMaxStampFrames));
    unsigned long long *d_stamps = v->d_stamps;
    auto stamp = [&](hipStream_t st, int frame, int slot) {
        if (stamps && frame < kMaxStampFrames)
            hipLaunchKernelGGL(stamp_kernel, dim3(1), dim3(1), 0, st, d_stamps + 8 * frame + slot);
    };
    svo_pyramid *ref = v->pyr_ref, *cur = v->pyr_cur, *nxt = v->pyr_next;
    svo_pyramid *right[2] = {v->pyr_right, v->pyr_right2};
    const int *run = &v->d_chain->run;
    const int frame0 = v->frame, nf = r.n_frames;
    struct OnStream {  // the launch helpers take the stream from the context
        svo_ctx *c;
        hipStream_t keep;
        OnStream(svo_ctx *cc, hipStream_t st) : c(cc), keep(cc->stream) { c->stream = st; }
        ~OnStream() { c->stream = keep; }
    };
    // pyramids of frame g of the run on D (the left one into `left`)
    auto pyramids = [&](int g, svo_pyramid *left) -> int {
        const uint8_t *li = r.lefts[g], *ri = r.rights[g];
        svo_pyramid *rp = right[g & 1];
        OnStream on(ctx, sD);
        if ((rc = build_pyramids(ctx, 1, &v, &left, &rp, &li, &ri)))
            return rc;
        SVO_HIP(hipEventRecord(ev[EV_PYR + (g & 3)], sD));
        return SVO_OK;
    };
    // the stereo path of frame g on C, from the pyramids D has built
    auto stereo = [&](int g, svo_pyramid *left) -> int {
        SVO_HIP(hipStreamWaitEvent(sC, ev[EV_PYR + (g & 3)], 0));
        if ((rc = stereo_part1_spec(v, left, right[g & 1], frame0 + g + 1, g % 3)))
            return rc;
        SVO_HIP(hipEventRecord(ev[EV_C + (g & 3)], sC));
        return SVO_OK;
    };
    // ... and its triangulation, on D
    auto triangulate = [&](int g) -> int {
        SVO_HIP(hipStreamWaitEvent(sD, ev[EV_C + (g & 3)], 0));
        {
            OnStream on(ctx, sD);
            if ((rc = stereo_tri_spec(v, g % 3)))
                return rc;
        }
        SVO_HIP(hipEventRecord(ev[EV_P1 + (g & 3)], sD));
        return SVO_OK;
    };
    // E: the tracking pass into frame g from the 2-D points the stereo path of frame g-1 has left -- what frame g starts
    // from if g-1 turns out to be a keyframe.  Nothing in it depends on a decision or a tracked set: it runs as soon as
    // that stereo path and the pyramids of g exist, a frame and a half before the filters that may read it.
    auto kf_pass = [&](int g, svo_pyramid *from, svo_pyramid *into) -> int {
        SVO_HIP(hipStreamWaitEvent(sE, ev[EV_C + ((g - 1) & 3)], 0));  // the 2-D points of that stereo path
        SVO_HIP(hipStreamWaitEvent(sE, ev[EV_PYR + (g & 3)], 0));
        const LkJob q = lk_job(from, into, v->h_x1[(g - 1) % 3], v->cap, v->h_cnt + (g - 1) % 3, v->a2k[g % 3], v->statusk[g % 3],
                               nullptr, run);
        {
            OnStream on(ctx, sE);
            if ((rc = svo_launch_lk_batch(ctx, 1, &q, from)))
                return rc;
        }
        SVO_HIP(hipEventRecord(ev[EV_E + (g & 3)], sE));
        return SVO_OK;
    };
    // prologue: the chain state is on its way (chain_prepare, on A); the pyramids of frames 0 and 1, the tracking
    // pass into frame 0 from the reference set, the stereo paths of frames 0 and 1, the keyframe pass into frame 1
    SVO_HIP(hipEventRecord(ev[EV_FLT], sA));
    SVO_HIP(hipStreamWaitEvent(sD, ev[EV_FLT], 0));
    if ((rc = pyramids(0, cur)) || (nf > 1 && (rc = pyramids(1, nxt))))
        return rc;
    {
        SVO_HIP(hipStreamWaitEvent(sA, ev[EV_PYR], 0));
        const float *pts = v->ref2d;
        const int *dn = &v->d_chain->nref;
        if ((rc = chain_lk(ctx, 1, &v, &ref, &cur, &pts, &dn, &run)))
            return rc;
        if ((rc = stereo(0, cur)) || (nf > 1 && (rc = stereo(1, nxt))) || (rc = triangulate(0)) ||
            (nf > 1 && (rc = kf_pass(1, cur, nxt))))
            return rc;
    }
    if (nf > 1)
        SVO_HIP(hipStreamWaitEvent(sA, ev[EV_PYR + 1], 0));  // the first tracking launch's target
    for (int f = 0; f < nf; f++) {
        v->frame++;
        const int set = f & 1, slot = f % 3;
        const bool more = f + 1 < nf;
        stamp(sA, f, 0);
        // the 2-D half of the filters; the previous frame a keyframe: from the sets of the pass that started at its points
        if ((rc = chain_filters(ctx, 1, &v, set, (f + 2) % 3, f & 1, f % 3)))
            return rc;
        SVO_HIP(hipEventRecord(ev[EV_FLT], sA));
        stamp(sA, f, 1);
        // B: the 3-D column of the filters, hypotheses, the decision (all A waits for); then a keyframe is refined and
        // its sets handed over; any other frame is refined after that.  (In order on B: the next frame's 3-D column
        // follows the hand-over it reads, its hypotheses follow this frame's refinement, which reads the workspace
        // they are written to.)
        SVO_HIP(hipStreamWaitEvent(sB, ev[EV_FLT], 0));
        {
            OnStream on(ctx, sB);
            stamp(sB, f, 3);
            if ((rc = chain_filters_3d(ctx, v, set, f & 1, f % 3)) || (rc = chain_pnp(ctx, 1, &v, set, true)))
                return rc;
            SVO_HIP(hipEventRecord(ev[EV_DEC], sB));
            stamp(sB, f, 4);
            SVO_HIP(hipStreamWaitEvent(sB, ev[EV_P1 + (f & 3)], 0));  // the stereo path of this frame: long done
            if ((rc = chain_pnp_refine(ctx, v, set, true)) || (rc = stereo_part2_spec(v, cur, slot, 3)))
                return rc;
            stamp(sB, f, 5);
            SVO_HIP(hipEventRecord(ev[EV_P3 + (f & 3)], sB));
            if ((rc = chain_pnp_refine(ctx, v, set, false)))
                return rc;
        }
        // D: the pyramids of frame f+2 into the buffer of frame f-1, whose last readers were the tracking launch of
        // the previous iteration (before these filters on A), the stereo path of frame f-1 (C is in order: frame f's
        // is done) and the colours of keyframe f-1 (its hand-over on B); the right pyramid it overwrites is the one
        // the stereo path of frame f has read
        if (more) {
            SVO_HIP(hipStreamWaitEvent(sD, ev[EV_FLT], 0));
            SVO_HIP(hipStreamWaitEvent(sD, ev[EV_C + (f & 3)], 0));
            if (f > 0)  // ... and the hand-over of keyframe f-2 (B is in order), whose cloud's buffer the triangulation below writes
                SVO_HIP(hipStreamWaitEvent(sD, ev[EV_P3 + ((f - 1) & 3)], 0));
            if (f + 2 < nf && (rc = pyramids(f + 2, ref)))
                return rc;
            if ((rc = triangulate(f + 1)))  // the stereo path of the next frame ends here (its 2-D part is long done)
                return rc;
        }
        if (more) {  // A: the tracking pass into frame f+1 from the tracked set
            const TrackedSet ts = tracked_set(v, set);
            const LkJob q = lk_job(cur, nxt, ts.p2, v->cap, ts.cnt, v->a2, (f + 1) & 1 ? v->status_b : v->status, nullptr, run);
            if ((rc = svo_launch_lk_batch(ctx, 1, &q, cur)))
                return rc;
            stamp(sA, f, 2);
            SVO_HIP(hipEventRecord(ev[EV_LK], sA));
            // C: the stereo path of frame f+2 once this launch has ended.  It writes the hand-over set of frame f-1,
            // whose readers were the previous iteration's launch and that frame's hand-over on B.
            if (f + 2 < nf) {
                SVO_HIP(hipStreamWaitEvent(sC, ev[EV_LK], 0));
                if (f > 0)
                    SVO_HIP(hipStreamWaitEvent(sC, ev[EV_P3 + ((f - 1) & 3)], 0));
                stamp(sC, f, 6);
                if ((rc = stereo(f + 2, ref)))  // `ref`: where D has just been told to build frame f+2
                    return rc;
                stamp(sC, f, 7);
                // E: the keyframe pass from frame f+1 into frame f+2, when A's launch has ended too.  Its output
                // buffer (target % 3) was last read by the filters of frame f-1 on A and B, before the decision A
                // waited for at the end of the previous iteration.
                SVO_HIP(hipStreamWaitEvent(sE, ev[EV_LK], 0));
                if ((rc = kf_pass(f + 2, nxt, ref)))
                    return rc;
            }
        }
        // What the next iteration needs of the streams that run ahead is waited for HERE, before the wait for the
        // decision: every wait is a barrier packet of ~7 us on the stream, and while B decides this stream is idle
        // anyway -- after the decision nothing but the filters' launches is left.
        if (f + 2 < nf)
            SVO_HIP(hipStreamWaitEvent(sA, ev[EV_PYR + ((f + 2) & 3)], 0));  // the next tracking launch's target
        if (more)
            SVO_HIP(hipStreamWaitEvent(sA, ev[EV_E + ((f + 1) & 3)], 0));    // the keyframe pass the next filters may read
        SVO_HIP(hipStreamWaitEvent(sA, ev[EV_DEC], 0));  // the next filters: the keyframe flag, a plain frame's 2-D set
        svo_pyramid *t = ref;  // referenceImg = currentImage (src/VisualSLAM.cpp:151)
        ref = cur;
        cur = nxt;
        nxt = t;
    }
    // the last frame's refinement runs on B: the caller's wait on A covers it
    SVO_HIP(hipEventRecord(ev[EV_REF], sB));
    SVO_HIP(hipStreamWaitEvent(sA, ev[EV_REF], 0));
    if (stamps && nf > 40)
        return chain_read_stamps(v, nf, stamps_env);
    return SVO_OK;
}

// Queue frames [0, n) of k chunks that share a context in lock step on its stream: every stage one set of launches for
// all of them; chunks may differ in length.
static int chain_enqueue_lockstep(ChainRun *const *runs, int k)
{
    svo_vo *v0 = runs[0]->v;
    svo_ctx *ctx = v0->ctx;
    int n_max = 0, rc;
    for (int a = 0; a < k; a++)
        n_max = runs[a]->n_frames > n_max ? runs[a]->n_frames : n_max;
    if (n_max == 0)
        return SVO_OK;
    svo_vo *vs[SVO_LK_MAX_JOBS];
    svo_pyramid *prevs[SVO_LK_MAX_JOBS], *nexts[SVO_LK_MAX_JOBS];
    const float *pts[SVO_LK_MAX_JOBS];
    const int *dn[SVO_LK_MAX_JOBS], *gates[SVO_LK_MAX_JOBS];
    svo_pyramid *ref[SVO_LK_MAX_JOBS], *cur[SVO_LK_MAX_JOBS];
    for (int a = 0; a < k; a++) {
        ref[a] = runs[a]->v->pyr_ref;
        cur[a] = runs[a]->v->pyr_cur;
    }
    // Host images (KITTI replay: the frames are in host memory): the library uploads them itself, on a copy stream of the
    // context, TWO STEPS AHEAD of the step that computes -- a ring of three device slots, each one step's left and right
    // images of every chunk of the group; the compute stream waits for a slot's upload, the copy stream for the slot's
    // previous pyramids.  Pinned host memory makes the uploads asynchronous; pageable memory works (the copies then block
    // the enqueuing thread).
    const bool host_imgs = runs[0]->mem == SVO_MEM_HOST;
    const size_t img_bytes = (size_t)v0->w * v0->h * v0->c;
    bool slot_used[3] = {false, false, false};
    auto slot_ptr = [&](int slot, int a, int side) {
        return ctx->up_ring.as<uint8_t>() + ((size_t)(slot * k + a) * 2 + side) * img_bytes;
    };
    auto upload_step = [&](int f) -> int {
        const int slot = f % 3;
        if (slot_used[slot])
            SVO_HIP(hipStreamWaitEvent(ctx->up_stream, ctx->use_ev[slot], 0));
        for (int a = 0; a < k; a++) {
            if (f >= runs[a]->n_frames)
                continue;
            SVO_HIP(hipMemcpyAsync(slot_ptr(slot, a, 0), runs[a]->lefts[f], img_bytes, hipMemcpyHostToDevice, ctx->up_stream));
            SVO_HIP(hipMemcpyAsync(slot_ptr(slot, a, 1), runs[a]->rights[f], img_bytes, hipMemcpyHostToDevice, ctx->up_stream));
        }
        SVO_HIP(hipEventRecord(ctx->up_ev[slot], ctx->up_stream));
        return SVO_OK;
    };
    if (host_imgs) {
        if (!ctx->up_stream) {
            SVO_HIP(hipStreamCreateWithFlags(&ctx->up_stream, hipStreamNonBlocking));
            for (int s3 = 0; s3 < 3; s3++) {
                SVO_HIP(hipEventCreateWithFlags(&ctx->up_ev[s3], hipEventDisableTiming));
                SVO_HIP(hipEventCreateWithFlags(&ctx->use_ev[s3], hipEventDisableTiming));
            }
        }
        if ((rc = ctx->up_ring.ensure((size_t)3 * k * 2 * img_bytes)))
            return rc;
        // what the group's stream has queued so far may still read the ring (a run that was resumed): order behind it
        SVO_HIP(hipEventRecord(ctx->use_ev[0], ctx->stream));
        SVO_HIP(hipStreamWaitEvent(ctx->up_stream, ctx->use_ev[0], 0));
        if ((rc = upload_step(0)) || (n_max > 1 && (rc = upload_step(1))))
            return rc;
    }
    for (int f = 0; f < n_max; f++) {
        int na = 0, idx[SVO_LK_MAX_JOBS];
        svo_pyramid *rp[SVO_LK_MAX_JOBS];
        const uint8_t *li[SVO_LK_MAX_JOBS], *ri[SVO_LK_MAX_JOBS];
        for (int a = 0; a < k; a++) {
            if (f >= runs[a]->n_frames)
                continue;
            svo_vo *v = runs[a]->v;
            v->frame++;
            idx[na] = a;
            vs[na] = v;
            prevs[na] = ref[a];
            nexts[na] = cur[a];
            rp[na] = v->pyr_right;
            li[na] = host_imgs ? slot_ptr(f % 3, a, 0) : runs[a]->lefts[f];
            ri[na] = host_imgs ? slot_ptr(f % 3, a, 1) : runs[a]->rights[f];
            pts[na] = v->ref2d;
            dn[na] = &v->d_chain->nref;
            gates[na] = &v->d_chain->run;
            na++;
        }
        if (na == 0)
            break;
        float *o2[SVO_LK_MAX_JOBS], *o3[SVO_LK_MAX_JOBS];
        const double *noRt[SVO_LK_MAX_JOBS];
        int *non[SVO_LK_MAX_JOBS];
        for (int a = 0; a < na; a++) {
            o2[a] = vs[a]->ref2d;
            o3[a] = vs[a]->ref3d;
            noRt[a] = nullptr;
            non[a] = nullptr;
        }
        if (host_imgs) {
            if (f + 2 < n_max && (rc = upload_step(f + 2)))
                return rc;
            SVO_HIP(hipStreamWaitEvent(ctx->stream, ctx->up_ev[f % 3], 0));
        }
        if ((rc = build_pyramids(ctx, na, vs, nexts, rp, li, ri)))
            return rc;
        if (host_imgs) {   // the slot's images are in the pyramids now (colours come from level 0): it may be overwritten
            SVO_HIP(hipEventRecord(ctx->use_ev[f % 3], ctx->stream));
            slot_used[f % 3] = true;
        }
        if ((rc = chain_lk(ctx, na, vs, prevs, nexts, pts, dn, gates)) || (rc = chain_filters(ctx, na, vs)) ||
            (rc = chain_pnp(ctx, na, vs)) || (rc = stereo_triangulate_batch(na, vs, nexts, rp, noRt, o2, o3, non, true)))
            return rc;
        for (int a = 0; a < na; a++)
            std::swap(ref[idx[a]], cur[idx[a]]);
    }
    return SVO_OK;
}

// pipeline: one chunk, device images
static int chain_enqueue(ChainRun *const *runs, int k, bool pipeline)
{
    return pipeline ? chain_enqueue_pipelined(*runs[0]) : chain_enqueue_lockstep(runs, k);
}

// after the stream has drained: the chain state and the per-frame records of one chunk, the host mirror of the state
static int chain_collect(ChainRun &r, bool pipeline)
{
    svo_vo *v = r.v;
    svo_ctx *ctx = v->ctx;
    SVO_HIP(hipMemcpyAsync(v->h_chain, v->d_chain, sizeof(VoChain), hipMemcpyDeviceToHost, ctx->stream));
    int rc = svo_wait(ctx);
    if (rc)
        return rc;
    r.end = *v->h_chain;
    const int done = r.end.frame < r.n_frames ? r.end.frame : r.n_frames;
    for (int f = 0; f < done; f++) {
        const VoOut &o = v->h_out[f];
        memcpy(r.R_out + 9 * (size_t)f, o.R, sizeof(o.R));
        memcpy(r.t_out + 3 * (size_t)f, o.t, sizeof(o.t));
        if (r.inliers_out)
            r.inliers_out[f] = o.inliers;
        if (r.tracked_out)
            r.tracked_out[f] = o.tracked;
        if (r.keyframe_out)
            r.keyframe_out[f] = (uint8_t)o.keyframe;
    }
    r.n_done = done;
    r.halt_set = pipeline ? (r.end.frame & 1) : 0;  // pipelined chunks alternate between two tracked sets
    // host mirror of the device state after `done` frames
    v->nref = r.end.nref;
    v->kf_n = r.end.kf_n;
    if (done > 0) {
        memcpy(v->R, r.end.R, sizeof(v->R));
        memcpy(v->t, r.end.t, sizeof(v->t));
    }
    v->frame = r.frame0 + done;
    svo_pyramid *p[3] = {r.p0, r.p1, r.p2};
    // a frame that halted in its PnP has its pyramid built (it is `cur`); the roles after `done` finished frames
    if (pipeline) {
        v->pyr_ref = p[done % 3];
        v->pyr_cur = p[(done + 1) % 3];
        v->pyr_next = p[(done + 2) % 3];
    } else {
        v->pyr_ref = p[done % 2];
        v->pyr_cur = p[(done + 1) % 2];
    }
    v->has_cur = false;
    return SVO_OK;
}

// The chain stopped in the PnP of frame h with fewer than 10 inliers at 1 px (SVO_HALT_RETRY): the host runs
// PerspectiveNpointEstimation's second attempt (100, 8.0, 0.98; src/keyFrameManagement.cpp:85-92) on the tracked sets
// the chain left in place, then the frame's policy as svo_vo_update does.  v->frame is the halted frame's number.
static int chain_retry_frame(ChainRun &r, int h)
{
    svo_vo *v = r.v;
    svo_ctx *ctx = v->ctx;
    int rc;
    v->frame = r.frame0 + h + 1;
    if (r.halt_set) {  // the frame wrote the second tracked set: make it the front-end's (svo_vo_update swaps pointers)
        std::swap(v->trk2d, v->trk2d_b);
        std::swap(v->trk3d, v->trk3d_b);
    }
    const int *cnt = tracked_set(v, r.halt_set).cnt;
    const double K4[4] = {v->prm.fx, v->prm.fy, v->prm.cx, v->prm.cy};
    const PnpRecord *rec = reinterpret_cast<const PnpRecord *>(ctx->pinned);
    const TrackedSet ts = tracked_set(v, 0);  // the front-end's own set: after the swap, the points the frame wrote
    if ((rc = svo_launch_pnp_ransac(ctx, ts.p3, ts.p2, v->cap, cnt, K4, 100, 8.0, 0.98, stage_seed(v, v->frame, 2), 20, ts.idx,
                                    nullptr, ts.rec)) ||
        (rc = vo_fetch_record(ctx, ts.rec, cnt)))
        return rc;
    v->ntrk = rec->n_tracked;
    if (r.inliers_out)
        r.inliers_out[h] = rec->n_inliers;
    if (r.tracked_out)
        r.tracked_out[h] = rec->n_tracked;
    if (rec->n_inliers < v->prm.pnp_lost_below) {
        svo_set_error("tracking lost at frame %d: %d PnP inliers", v->frame, rec->n_inliers);
        return SVO_ERR_TRACKING_LOST;
    }
    double *R9 = r.R_out + 9 * (size_t)h, *t3 = r.t_out + 3 * (size_t)h;
    pose_from_record(*rec, R9, t3);
    int was_kf = 0;
    v->has_cur = true;  // the chain built this frame's pyramid: it is pyr_cur
    if ((rc = svo_vo_update(v, r.rights[h], r.mem, R9, t3, rec->n_inliers, 0, &was_kf)))
        return rc;
    if (r.keyframe_out)
        r.keyframe_out[h] = (uint8_t)was_kf;
    return SVO_OK;
}

// Runs k chunks that share a context to the end: queue, wait, collect; a chunk whose chain halted is taken to the end
// on its own (the slow paths are rare; the other chunks of the set are not held up by it).
static int chain_run(ChainRun *const *runs, int k, bool pipeline)
{
    int rc;
    svo_ctx *ctx = runs[0]->v->ctx;
    for (int a = 0; a < k; a++)
        if ((rc = chain_prepare(*runs[a])))
            return rc;
    static const bool debug = getenv("SVO_CHAIN_DEBUG") != nullptr;  // host time of the enqueue against the device's
    const auto t0 = std::chrono::steady_clock::now();
    if ((rc = chain_enqueue(runs, k, pipeline)))
        return rc;
    const auto t1 = std::chrono::steady_clock::now();
    if ((rc = svo_wait(ctx)))
        return rc;
    if (debug) {
        const auto t2 = std::chrono::steady_clock::now();
        fprintf(stderr, "[svo chain] %d chunk(s) x %d frames, pipeline %d: enqueue %.1f us, then waited %.1f us\n", k,
                runs[0]->n_frames, (int)pipeline, std::chrono::duration<double, std::micro>(t1 - t0).count(),
                std::chrono::duration<double, std::micro>(t2 - t1).count());
    }
    for (int a = 0; a < k; a++)
        if ((rc = chain_collect(*runs[a], pipeline)))
            return rc;
    if (getenv("SVO_CHAIN_DRY"))  // experiment (see chain_prepare): nothing ran, report the frames as done
        for (int a = 0; a < k; a++)
            runs[a]->n_done = runs[a]->n_frames;
    for (int a = 0; a < k; a++) {
        ChainRun &r = *runs[a];
        svo_vo *v = r.v;
        while (r.n_done < r.n_frames && r.rc == SVO_OK) {
            if (r.end.halt_code == SVO_HALT_FEW_REF || (r.end.halt_code == SVO_HALT_NONE && v->nref < 5)) {
                svo_set_error("tracking lost: %d reference points", v->nref);
                r.rc = SVO_ERR_TRACKING_LOST;
                break;
            }
            if (r.end.halt_code != SVO_HALT_RETRY) {
                svo_set_error("front-end chain stopped after %d of %d frames without a reason", r.n_done, r.n_frames);
                return SVO_ERR_STATE;
            }
            const int h = r.n_done;
            rc = chain_retry_frame(r, h);
            if (rc == SVO_ERR_TRACKING_LOST) {
                r.rc = rc;
                break;
            }
            if (rc)
                return rc;
            // the rest of the chunk as a run of its own
            ChainRun rest = r;
            rest.lefts = r.lefts + h + 1;
            rest.rights = r.rights + h + 1;
            rest.n_frames = r.n_frames - h - 1;
            rest.R_out = r.R_out + 9 * (size_t)(h + 1);
            rest.t_out = r.t_out + 3 * (size_t)(h + 1);
            rest.inliers_out = r.inliers_out ? r.inliers_out + h + 1 : nullptr;
            rest.tracked_out = r.tracked_out ? r.tracked_out + h + 1 : nullptr;
            rest.keyframe_out = r.keyframe_out ? r.keyframe_out + h + 1 : nullptr;
            r.n_done = h + 1;
            if (rest.n_frames == 0)
                break;
            if ((r.rc = vo_check_reference(v->nref)))
                break;
            ChainRun *one = &rest;
            if ((rc = chain_prepare(rest)) || (rc = chain_enqueue(&one, 1, pipeline)) || (rc = svo_wait(ctx)) ||
                (rc = chain_collect(rest, pipeline)))
                return rc;
            r.n_done = h + 1 + rest.n_done;
            r.end = rest.end;
            r.halt_set = rest.halt_set;
        }
    }
    return SVO_OK;
}

extern "C" {

int svo_vo_run_chunk(svo_vo *v, const uint8_t *const *lefts, const uint8_t *const *rights, int n_frames, int mem,
                     int pipeline, double *R_out, double *t_out, int *inliers_out, int *tracked_out,
                     uint8_t *keyframe_out, int *n_done)
{
    SVO_CHECK_ARG(v && lefts && rights && n_frames >= 0 && R_out && t_out);
    SVO_CHECK_ARG(mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE);
    if (v->prm.policy != SVO_POLICY_SLAM) {
        svo_set_error("the chunk runner drives the live policy (SVO_POLICY_SLAM) only");
        return SVO_ERR_ARG;
    }
    if (n_done)
        *n_done = 0;
    if (n_frames == 0)
        return SVO_OK;
    SVO_HIP(hipSetDevice(v->ctx->device));
    if (mem == SVO_MEM_HOST)
        pipeline = 0;  // host images go through the lock-step runner's upload ring
    int rc;
    if ((pipeline && (rc = vo_pipe_prepare(v))) || (rc = vo_check_reference(v->nref)))
        return rc;
    ChainRun r = make_run(v, lefts, rights, n_frames, mem, R_out, t_out, inliers_out, tracked_out, keyframe_out);
    ChainRun *one = &r;
    rc = chain_run(&one, 1, pipeline != 0);
    if (n_done)
        *n_done = r.n_done;
    return rc ? rc : r.rc;
}

// Several chunks that share ONE context, advanced in lock step by one host thread on the context's
// stream: per frame the pyramids of all of them, ONE pyramidal-LK launch carrying all their
// tracking passes (the launch lasts as long as its slowest keypoint, so k jobs cost little more
// than one), then each stage of the chain as one set of launches.  Every chunk gets exactly what
// svo_vo_run_chunk(pipeline = 0) gives it alone.
static int run_chunk_group(svo_chunk_job **jobs, int k)
{
    svo_ctx *ctx = jobs[0]->vo->ctx;
    int rc;
    for (int a = 0; a < k; a++) {
        jobs[a]->n_done = 0;
        jobs[a]->rc = SVO_OK;
        if (jobs[a]->mem != jobs[0]->mem) {
            svo_set_error("chunks that share a context take their images from the same side (all host or all device)");
            return SVO_ERR_ARG;
        }
        if (jobs[a]->vo->prm.policy != SVO_POLICY_SLAM) {
            svo_set_error("the chunk runner drives the live policy (SVO_POLICY_SLAM) only");
            return SVO_ERR_ARG;
        }
        if (!jobs[a]->init_left != !jobs[a]->init_right) {
            svo_set_error("svo_vo_run_chunks: init_left and init_right go together");
            return SVO_ERR_ARG;
        }
    }
    {   // ---- chunks that start here: svo_vo_init of all of them as one set of launches ----
        svo_vo *vs[SVO_LK_MAX_JOBS];
        svo_pyramid *pl[SVO_LK_MAX_JOBS], *pr[SVO_LK_MAX_JOBS];
        const uint8_t *il[SVO_LK_MAX_JOBS], *ir[SVO_LK_MAX_JOBS];
        const double *Rts[SVO_LK_MAX_JOBS];
        float *o2d[SVO_LK_MAX_JOBS], *o3d[SVO_LK_MAX_JOBS];
        int *nout[SVO_LK_MAX_JOBS];
        int ni = 0;
        for (int a = 0; a < k; a++) {
            svo_chunk_job *j = jobs[a];
            if (!j->init_left)
                continue;
            svo_vo *v = j->vo;
            v->frame = 0;
            vo_reset_pose(v);
            v->has_cur = false;
            vs[ni] = v;
            pl[ni] = v->pyr_ref;
            pr[ni] = v->pyr_right;
            il[ni] = j->init_left;
            ir[ni] = j->init_right;
            Rts[ni] = kIdentityRt;  // as svo_vo_init
            o2d[ni] = v->ref2d;
            o3d[ni] = v->ref3d;
            nout[ni] = &v->nref;
            ni++;
        }
        if (ni > 0 && jobs[0]->mem == SVO_MEM_HOST) {
            // host images: the initialisation's frames go through the upload ring's memory on the group's own stream (the
            // run's first uploads are ordered behind what this stream has queued, chain_enqueue_lockstep)
            svo_vo *v0 = jobs[0]->vo;
            const size_t img_bytes = (size_t)v0->w * v0->h * v0->c;
            if ((rc = ctx->up_ring.ensure((size_t)3 * k * 2 * img_bytes)))
                return rc;
            for (int a = 0; a < ni; a++) {
                uint8_t *dl = ctx->up_ring.as<uint8_t>() + (size_t)(2 * a) * img_bytes, *dr = dl + img_bytes;
                SVO_HIP(hipMemcpyAsync(dl, il[a], img_bytes, hipMemcpyHostToDevice, ctx->stream));
                SVO_HIP(hipMemcpyAsync(dr, ir[a], img_bytes, hipMemcpyHostToDevice, ctx->stream));
                il[a] = dl;
                ir[a] = dr;
            }
        }
        if (ni > 0) {
            if ((rc = svo_build_pyramids_from_device(ctx, ni, pl, il)) ||
                (rc = svo_build_pyramids_from_device(ctx, ni, pr, ir)) ||
                (rc = stereo_triangulate_batch(ni, vs, pl, pr, Rts, o2d, o3d, nout)))
                return rc;
            for (int a = 0; a < k; a++)
                if (jobs[a]->init_left)
                    jobs[a]->n_init_points = jobs[a]->vo->nref;
        }
    }
    ChainRun runs[SVO_LK_MAX_JOBS];
    ChainRun *rp[SVO_LK_MAX_JOBS];
    int nr = 0;
    for (int a = 0; a < k; a++) {
        svo_chunk_job *j = jobs[a];
        if (j->n_frames <= 0)
            continue;
        if ((j->rc = vo_check_reference(j->vo->nref)))
            continue;
        runs[nr] = make_run(j->vo, j->lefts, j->rights, j->n_frames, j->mem, j->R_out, j->t_out, j->inliers_out,
                            j->tracked_out, j->keyframe_out);
        rp[nr] = &runs[nr];
        nr++;
    }
    if (nr == 0)
        return SVO_OK;
    rc = chain_run(rp, nr, false);
    nr = 0;
    for (int a = 0; a < k; a++) {
        svo_chunk_job *j = jobs[a];
        if (j->n_frames <= 0 || j->rc)
            continue;
        j->n_done = runs[nr].n_done;
        j->rc = runs[nr].rc;
        nr++;
    }
    return rc;
}

int svo_vo_run_chunks(svo_chunk_job *jobs, int n_jobs)
{
    SVO_CHECK_ARG(jobs && n_jobs >= 1);
    // jobs that share a context form a group (lock step, one tracking launch for all of them);
    // every group runs on its own host thread
    std::vector<std::vector<svo_chunk_job *>> groups;
    for (int a = 0; a < n_jobs; a++) {
        SVO_CHECK_ARG(jobs[a].vo != nullptr);
        bool placed = false;
        for (auto &g : groups)
            if (g[0]->vo->ctx == jobs[a].vo->ctx) {
                for (svo_chunk_job *o : g)
                    if (o->vo == jobs[a].vo) {
                        svo_set_error("svo_vo_run_chunks: a front-end appears in two jobs");
                        return SVO_ERR_ARG;
                    }
                {  // a group's stages go out as one set of launches sized from its first member
                    const svo_vo *x = g[0]->vo, *y = jobs[a].vo;
                    const svo_vo_params &p = x->prm, &q = y->prm;
                    if (x->w != y->w || x->h != y->h || x->c != y->c || x->cap != y->cap || p.grid_step != q.grid_step ||
                        p.anms_keep != q.anms_keep || p.fx != q.fx || p.fy != q.fy || p.cx != q.cx || p.cy != q.cy ||
                        p.baseline != q.baseline) {
                        svo_set_error("svo_vo_run_chunks: the front-ends of one context must share image size, "
                                      "grid step, ANMS budget, intrinsics and baseline");
                        return SVO_ERR_ARG;
                    }
                }
                if ((int)g.size() >= SVO_LK_MAX_JOBS) {
                    svo_set_error("svo_vo_run_chunks: at most %d chunks per context", SVO_LK_MAX_JOBS);
                    return SVO_ERR_ARG;
                }
                g.push_back(&jobs[a]);
                placed = true;
                break;
            }
        if (!placed)
            groups.push_back({&jobs[a]});
    }
    const int ng = (int)groups.size();
    std::vector<std::string> errs(ng);
    std::vector<int> grc(ng, SVO_OK);
    auto body = [&](int gi) {
        auto &g = groups[gi];
        if (hipSetDevice(g[0]->vo->ctx->device) != hipSuccess) {  // the current device is per host thread
            grc[gi] = SVO_ERR_HIP;
            errs[gi] = "hipSetDevice failed";
            return;
        }
        if (g.size() == 1) {
            svo_chunk_job &j = *g[0];
            j.n_done = 0;
            if (!j.init_left != !j.init_right) {
                grc[gi] = SVO_ERR_ARG;
                errs[gi] = "svo_vo_run_chunks: init_left and init_right go together";
                return;
            }
            if (j.init_left && (j.rc = svo_vo_init(j.vo, j.init_left, j.init_right, j.mem, &j.n_init_points))) {
                grc[gi] = j.rc;
                errs[gi] = svo_last_error();
                return;
            }
            j.rc = svo_vo_run_chunk(j.vo, j.lefts, j.rights, j.n_frames, j.mem, j.pipeline, j.R_out, j.t_out,
                                    j.inliers_out, j.tracked_out, j.keyframe_out, &j.n_done);
            if (j.rc && j.rc != SVO_ERR_TRACKING_LOST)
                grc[gi] = j.rc;
        } else {
            grc[gi] = run_chunk_group(g.data(), (int)g.size());
        }
        if (grc[gi])
            errs[gi] = svo_last_error();  // the error text is thread-local
    };
    std::vector<std::thread> th;
    for (int gi = 1; gi < ng; gi++)
        th.emplace_back(body, gi);
    body(0);
    for (auto &t : th)
        t.join();
    for (int gi = 0; gi < ng; gi++)
        if (grc[gi]) {
            svo_set_error("chunk group %d: %s", gi, errs[gi].c_str());
            return grc[gi];
        }
    return SVO_OK;
}

}  // extern "C"
