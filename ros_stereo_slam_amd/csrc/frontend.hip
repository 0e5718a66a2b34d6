// frontend.hip -- the stereo-VO front-end frame loop on one GPU (svo_vo).
//
// Host-side mirror of visualSLAM::initSequence's per-frame body
// (src/VisualSLAM.cpp:11-169) with every data-parallel stage on the device:
//   svo_vo_init      stereoTriangulate of frame 0            VisualSLAM.cpp:22-41
//   svo_vo_localize  PerspectiveNpointEstimation + pose      VisualSLAM.cpp:64-74,
//                    composition                              keyFrameManagement.cpp:73-94
//   svo_vo_update    keyframe rule + reference hand-over     VisualSLAM.cpp:93-152,
//                                                             keyFrameManagement.cpp:9-31
// The split lets the caller run the pose graph between the two (VisualSLAM.cpp:76-89
// re-anchors t after a loop closure before the keyframe is inserted).
//
// Device residency: the reference image pyramid, the current pyramid, the reference point
// sets (2-D, 3-D world) and every intermediate live in HBM.  A localisation enqueues
// pyramid -> LK -> compaction -> F-RANSAC -> compaction -> PnP-RANSAC (+refine) on the
// context's stream with device-side counts chained between stages, and reads back ONE
// 144-byte record (pose, inlier count, tracked count) -- the values the reference's host
// policy branches on (inliers < 10: retry / shutdown; inliers < 200: keyframe).
#include <string>
#include <thread>
#include <vector>
#include <chrono>
#include <cmath>

#include "svo_internal.h"

struct PnpRecord {  // layout of pnp.hip's PnpResult + the tracked-point count behind it
    double rvec[3], tvec[3], R[9], rms;
    int n_inliers, iters_run;
    int n_tracked, pad;
};

struct svo_vo {
    svo_ctx *ctx = nullptr;
    svo_vo_params prm;
    int w = 0, h = 0, c = 0, cap = 0;
    svo_pyramid *pyr_ref = nullptr, *pyr_cur = nullptr, *pyr_right = nullptr, *pyr_next = nullptr, *pyr_right2 = nullptr;
    // One chunk per GPU, pipelined (svo_vo_run_chunk, pipeline != 0): four streams.
    //   A   the context's stream: the frame's filters, then BOTH tracking passes frame f+1 can start from -- from the
    //       tracked set (f is no keyframe) and from the 2-D points the stereo path of f has left (f is a keyframe) -- as one
    //       launch; the next filters take the one the decision points to
    //   B   stream_b: PnP hypotheses, the decision, the refinement (a keyframe's first, then the hand-over of its sets)
    //   C   lane.ctx: the whole stereo path of EVERY frame (LK left -> right, ANMS, filters, DLT triangulation in the
    //       camera frame: none of it needs the frame's pose), a frame ahead, on a context of its own (stream, scratch,
    //       tickets) with its own staging buffers
    //   D   stream_p: the pyramids, two frames ahead
    hipStream_t stream_b = nullptr, stream_p = nullptr;
    struct StereoLane {
        svo_ctx *ctx = nullptr;
        float *a2 = nullptr, *b2 = nullptr, *c2 = nullptr, *d2 = nullptr, *x2 = nullptr, *resp = nullptr;
        uint8_t *status = nullptr, *st2 = nullptr, *mask = nullptr;
        int *idx = nullptr, *cnt = nullptr;
    } lane;
    // what the lane hands to A and B, by frame % 3: the keyframe candidate's 2-D points, camera-frame points, count
    float *h_x1[3] = {nullptr, nullptr, nullptr}, *h_xyz[3] = {nullptr, nullptr, nullptr}, *h_x2[3] = {nullptr, nullptr, nullptr};
    int *h_cnt = nullptr;
    // output of the tracking pass from the keyframe candidate's points (beside a2 / status of the pass from the tracked set)
    float *a2k[3] = {nullptr, nullptr, nullptr};  // by target frame % 3 (stream E writes a frame's two frames ahead)
    // status bytes of both passes by frame parity: the PnP stream reads a frame's while A's next launch writes the next frame's
    uint8_t *statusk[3] = {nullptr, nullptr, nullptr}, *status_b = nullptr;
    // tracked sets ready (A), tracking launch ended (A), cloud placed (B), refined (B: end of a run); by frame & 3: pyramids
    // built (D), stereo path done (C)
    hipEvent_t ev_flt = nullptr, ev_lk = nullptr, ev_dec = nullptr, ev_ref = nullptr;
    hipEvent_t ev_pyr[4] = {nullptr, nullptr, nullptr, nullptr}, ev_p1[4] = {nullptr, nullptr, nullptr, nullptr},
               ev_p3[4] = {nullptr, nullptr, nullptr, nullptr}, ev_e[4] = {nullptr, nullptr, nullptr, nullptr}, ev_c[4] = {nullptr, nullptr, nullptr, nullptr};
    // the two hand-overs on a frame's critical path (tracked sets ready: A -> B; decided: B -> A) as stream memory
    // operations on signal memory (hipStreamWriteValue32 / hipStreamWaitValue32: half the latency of an event), values count up
    uint64_t *sig_flt = nullptr, *sig_dec = nullptr;
    uint32_t sig_n = 0;
    bool pipe_ready = false;
    // second set of tracked points / inlier list: frame t's refinement reads its set while frame t+1's filters write theirs
    float *trk2d_b = nullptr, *trk3d_b = nullptr;
    int *idx_b = nullptr;
    // point sets (device)
    float *ref2d = nullptr, *ref3d = nullptr, *trk2d = nullptr, *trk3d = nullptr;
    float *a2 = nullptr, *b2 = nullptr, *c2 = nullptr, *d2 = nullptr, *a3 = nullptr, *b3 = nullptr, *resp = nullptr;
    float *kf_col = nullptr;  // colours of the last keyframe's points (B, G, R as floats), beside its cloud in b3
    uint8_t *status = nullptr, *mask = nullptr, *st2 = nullptr;
    float *grid_xy = nullptr;  // the keypoint lattice of src/triangulation.cpp:89-96, written once at creation
    int *idx = nullptr, *d_cnt = nullptr;  // d_cnt[0..7]: stage counts
    PnpRecord *d_rec = nullptr;
    uint8_t *d_img = nullptr;  // staging for host images
    // the chain runner's device-resident frame state (svo_internal.h: VoChain), its pinned staging copy and the pinned
    // per-frame records the kernels fill
    VoChain *d_chain = nullptr, *h_chain = nullptr;
    VoOut *h_out = nullptr;
    int out_cap = 0;
    int nref = 0, ntrk = 0, frame = 0;
    int kf_n = 0;  // points of the last keyframe's camera-frame cloud in b3
    int ladder_ransac_inliers = 0;
    double R[9], t[3];
    bool has_cur = false;
    // svo_vo_set_stage_stamps: device time stamps between the stages of a pipelined run (8 per frame), read back into
    // stage_us by the run (mean intervals in microseconds over the middle of the run; stage_n = how many are valid)
    bool stamps_on = false;
    unsigned long long *d_stamps = nullptr;
    double stage_us[SVO_STAGE_COUNT] = {0};
    int stage_frames = 0;
};

namespace {

template <class T> int dev_alloc(T **p, size_t count)
{
    hipError_t e = hipMalloc((void **)p, count * sizeof(T));
    if (e != hipSuccess) {
        svo_set_error("hipMalloc(%zu) -> %s", count * sizeof(T), hipGetErrorString(e));
        return SVO_ERR_HIP;
    }
    return SVO_OK;
}

int grid_axis(int dim, int step)
{
    int k = 0;
    for (int v = step; v < dim - step; v += step)
        k++;
    return k;
}

uint64_t stage_seed(const svo_vo *v, int stage) { return v->prm.seed + 8ull * (uint64_t)v->frame + stage; }

__global__ void store_count_kernel(const int *__restrict__ src, int *__restrict__ dst) { *dst = *src; }

// debug (SVO_CHAIN_STAMPS): the constant 100 MHz clock, written by a one-lane launch between the stages of a stream
__global__ void stamp_kernel(unsigned long long *dst) { *dst = wall_clock64(); }

const uint8_t *stage_image(svo_vo *v, const uint8_t *img, int mem, int *rc)
{
    *rc = SVO_OK;
    if (mem == SVO_MEM_DEVICE)
        return img;
    hipError_t e =
        hipMemcpyAsync(v->d_img, img, (size_t)v->w * v->h * v->c, hipMemcpyHostToDevice, v->ctx->stream);
    if (e != hipSuccess) {
        svo_set_error("image upload -> %s", hipGetErrorString(e));
        *rc = SVO_ERR_HIP;
    }
    return v->d_img;
}

// visualSLAM::stereoTriangulate, dense branch (src/triangulation.cpp:87-103,137-165), with
// the optional ANMS stage, for k front-ends of one context at once (same image size, grid step
// and ANMS budget): every stage is one set of launches.  Per front-end: x1 -> out2d, camera-frame
// points -> v->b3 and, when Rt is given, world points -> out3d (else the camera-frame points).
// Count -> d_cnt[4] and host.
// chained: the chain runner's form -- every kernel of job a runs only when vs[a]->d_chain->kf is set, [R|t] is the
// pose the device holds (Rts ignored), the count goes to the chain state, nothing is waited for (n_out untouched).
int stereo_triangulate_batch(int k, svo_vo *const *vs, svo_pyramid *const *lefts, svo_pyramid *const *rights,
                             const double *const *Rts, float *const *out2d, float *const *out3d, int *const *n_out,
                             bool chained = false)
{
    svo_vo *v0 = vs[0];
    svo_ctx *ctx = v0->ctx;
    int rc;
    const int n = grid_axis(v0->w, v0->prm.grid_step) * grid_axis(v0->h, v0->prm.grid_step);
    LkJob lk[SVO_LK_MAX_JOBS];
    for (int a = 0; a < k; a++) {
        svo_vo *v = vs[a];
        // denseLKtracking: LK left -> right (src/tracking.cpp:18); min-eig is the ANMS response
        LkJob &q = lk[a];
        q.prev = lefts[a]->dev;
        q.next = rights[a]->dev;
        q.dprev = lefts[a]->dbase;
        q.prev_pts = v->grid_xy;
        q.n_cap = n;
        q.d_n = nullptr;
        q.next_pts = v->b2;
        q.status = v->status;
        q.err = nullptr;
        q.min_eig = v->resp;
        q.gate = chained ? &v->d_chain->kf : nullptr;
    }
    if ((rc = svo_launch_lk_batch(ctx, k, lk, lefts[0])))
        return rc;
    const int *gates[SVO_LK_MAX_JOBS];
    for (int a = 0; a < k; a++)
        gates[a] = chained ? &vs[a]->d_chain->kf : nullptr;
    const float *pts[SVO_LK_MAX_JOBS], *trk[SVO_LK_MAX_JOBS];
    const uint8_t *stt[SVO_LK_MAX_JOBS];
    const int *d_n[SVO_LK_MAX_JOBS];
    for (int a = 0; a < k; a++) {
        pts[a] = vs[a]->grid_xy;
        trk[a] = vs[a]->b2;
        stt[a] = vs[a]->status;
        d_n[a] = nullptr;
    }
    if (v0->prm.anms_keep > 0) {
        const float *xy[SVO_LK_MAX_JOBS], *resp[SVO_LK_MAX_JOBS];
        int *oidx[SVO_LK_MAX_JOBS], *ocnt[SVO_LK_MAX_JOBS];
        svo_anms_gather ga[SVO_LK_MAX_JOBS];
        for (int a = 0; a < k; a++) {
            svo_vo *v = vs[a];
            xy[a] = v->grid_xy;
            resp[a] = v->resp;
            oidx[a] = v->idx;
            ocnt[a] = v->d_cnt + 2;
            ga[a] = {v->grid_xy, v->b2, v->c2, v->d2, v->status, v->st2};
        }
        // the kept keypoints' lattice points, tracked points and status bytes come out of the same launch
        // that lists them (a gather launch of its own before)
        if ((rc = svo_launch_anms_batch(ctx, k, xy, resp, n, v0->prm.anms_keep, oidx, ocnt, ga, chained ? gates : nullptr)))
            return rc;
        for (int a = 0; a < k; a++) {
            pts[a] = vs[a]->c2;
            trk[a] = vs[a]->d2;
            stt[a] = vs[a]->st2;
            d_n[a] = vs[a]->d_cnt + 2;
        }
    }
    // status compaction (src/tracking.cpp:20-27); ping-pong between the (a2,b2) and (c2,d2) pairs
    svo_compact_job c1[SVO_LK_MAX_JOBS], c2[SVO_LK_MAX_JOBS];
    svo_fransac_job fj[SVO_LK_MAX_JOBS];
    svo_tri_job tj[SVO_LK_MAX_JOBS];
    for (int a = 0; a < k; a++) {
        svo_vo *v = vs[a];
        float *o1 = pts[a] == v->grid_xy ? v->c2 : v->a2, *o2 = pts[a] == v->grid_xy ? v->d2 : v->b2;
        float *x1 = out2d[a], *x2 = o1 == v->a2 ? v->c2 : v->a2;
        c1[a] = {stt[a], n, d_n[a], {pts[a], trk[a], nullptr}, {o1, o2, nullptr}, {2, 2, 0}, v->d_cnt + 3, gates[a]};
        // FmatThresholding (src/tracking.cpp:30-43): 3 px, 0.99
        c2[a] = {v->mask, n, v->d_cnt + 3, {o1, o2, nullptr}, {x1, x2, nullptr}, {2, 2, 0}, v->d_cnt + 4};
        fj[a] = {o1, o2, n, v->d_cnt + 3, v->prm.f_thr_stereo, 0.99, 1000, stage_seed(v, 3), v->mask, nullptr, nullptr,
                 nullptr, &c2[a], gates[a]};  // the mask compaction rides with the F-RANSAC
        if (chained)  // [R|t] and the gate come from the chain state; the count goes there
            tj[a] = {x1, x2, n, v->d_cnt + 4, v->b3, nullptr, nullptr, out3d[a], nullptr, v->d_chain};
        else
            tj[a] = {x1, x2, n, v->d_cnt + 4, Rts[a] ? v->b3 : out3d[a], nullptr, Rts[a], Rts[a] ? out3d[a] : nullptr,
                     reinterpret_cast<int *>(ctx->pinned) + a};  // the count the host reads after the wait below
        tj[a].color_src = lefts[a];  // `colors` of stereoTriangulate (src/triangulation.cpp:139-140), same launch
        tj[a].color_out = v->kf_col;
    }
    double P1[12], P2[12];
    svo_stereo_projections(v0->prm.fx, v0->prm.fy, v0->prm.cx, v0->prm.cy, v0->prm.baseline, P1, P2);
    if ((rc = svo_launch_compact_batch(ctx, k, c1)) || (rc = svo_launch_fransac_batch(ctx, k, fj)) ||
        (rc = svo_launch_triangulate_batch(ctx, P1, P2, k, tj)))
        return rc;
    if (chained)
        return SVO_OK;
    int *pin = reinterpret_cast<int *>(ctx->pinned);
    if ((rc = svo_wait(ctx)))
        return rc;
    for (int a = 0; a < k; a++) {
        *n_out[a] = pin[a];
        vs[a]->kf_n = Rts[a] ? pin[a] : 0;  // b3 holds the keyframe's camera-frame cloud
    }
    return SVO_OK;
}

// The stereo path of a keyframe candidate for ONE pipelined chunk, on a lane's stream and buffers: LK left -> right from
// the lattice (src/tracking.cpp:18), ANMS, status filter (:20-27), F-RANSAC at 3 px with its mask filter (:30-43), the
// DLT triangulation in the camera frame (src/triangulation.cpp:142-160) -- all of stereoTriangulate, none of which
// needs the frame's pose.  Leaves x1 / camera-frame points / count in h_x1 / h_xyz / h_cnt[slot].
// `frame_no`: the frame the pass belongs to (its seed).
int stereo_part1_spec(svo_vo *v, svo_vo::StereoLane &L, svo_pyramid *left, svo_pyramid *right, int frame_no, int slot)
{
    svo_ctx *cs = L.ctx;
    int rc;
    const int n = grid_axis(v->w, v->prm.grid_step) * grid_axis(v->h, v->prm.grid_step);
    const int *run = &v->d_chain->run;
    LkJob q;
    q.prev = left->dev;
    q.next = right->dev;
    q.dprev = left->dbase;
    q.prev_pts = v->grid_xy;
    q.n_cap = n;
    q.d_n = nullptr;
    q.next_pts = L.b2;
    q.status = L.status;
    q.err = nullptr;
    q.min_eig = L.resp;
    q.gate = run;
    if ((rc = svo_launch_lk_batch(cs, 1, &q, left)))
        return rc;
    const float *pts = v->grid_xy, *trk = L.b2;
    const uint8_t *stt = L.status;
    const int *d_n = nullptr;
    if (v->prm.anms_keep > 0) {
        const float *xy = v->grid_xy, *resp = L.resp;
        int *oidx = L.idx, *ocnt = L.cnt + 2;
        const svo_anms_gather ga = {v->grid_xy, L.b2, L.c2, L.d2, L.status, L.st2};
        if ((rc = svo_launch_anms_batch(cs, 1, &xy, &resp, n, v->prm.anms_keep, &oidx, &ocnt, &ga, &run)))
            return rc;
        pts = L.c2;
        trk = L.d2;
        stt = L.st2;
        d_n = L.cnt + 2;
    }
    float *o1 = pts == v->grid_xy ? L.c2 : L.a2, *o2 = pts == v->grid_xy ? L.d2 : L.b2;
    float *x1 = v->h_x1[slot];
    int *cnt = v->h_cnt + slot;
    const svo_compact_job c1 = {stt, n, d_n, {pts, trk, nullptr}, {o1, o2, nullptr}, {2, 2, 0}, L.cnt + 3, run};
    const svo_compact_job c2 = {L.mask, n, L.cnt + 3, {o1, o2, nullptr}, {x1, v->h_x2[slot], nullptr}, {2, 2, 0}, cnt};
    const uint64_t seed = v->prm.seed + 8ull * (uint64_t)frame_no + 3;  // stage_seed(frame_no, 3)
    const svo_fransac_job fj = {o1, o2, n, L.cnt + 3, v->prm.f_thr_stereo, 0.99, 1000, seed, L.mask, nullptr, nullptr,
                                nullptr, &c2, run};
    if ((rc = svo_launch_compact_batch(cs, 1, &c1)) || (rc = svo_launch_fransac_batch(cs, 1, &fj)))
        return rc;
    return SVO_OK;
}

// ... its last stage, the DLT triangulation of the filtered pairs in the camera frame (src/triangulation.cpp:142-160), on
// the context's current stream (the pipelined chunk runs it on the pyramid stream: the stereo stream is the busiest)
int stereo_tri_spec(svo_vo *v, int slot)
{
    const int n = grid_axis(v->w, v->prm.grid_step) * grid_axis(v->h, v->prm.grid_step);
    const svo_tri_job tj = {v->h_x1[slot], v->h_x2[slot], n, v->h_cnt + slot, v->h_xyz[slot], nullptr, nullptr, nullptr, nullptr};
    double P1[12], P2[12];
    svo_stereo_projections(v->prm.fx, v->prm.fy, v->prm.cx, v->prm.cy, v->prm.baseline, P1, P2);
    return svo_launch_triangulate_batch(v->ctx, P1, P2, 1, &tj);
}

// ... and what is left once the frame is decided, only when the device flag says keyframe: what = 1, the hand-over of
// the 2-D set (all the next tracking pass needs); what = 2, the cloud placed with the frame's refined pose
// (src/keyFrameManagement.cpp:18-30).  On the context's current stream.
int stereo_part2_spec(svo_vo *v, const svo_pyramid *left, int slot, int what)
{
    const int n = grid_axis(v->w, v->prm.grid_step) * grid_axis(v->h, v->prm.grid_step);
    return svo_launch_keyframe_place(v->ctx, v->d_chain, v->h_x1[slot], v->h_xyz[slot], n, v->h_cnt + slot, v->ref2d, v->b3,
                                     v->ref3d, left, v->kf_col, what);
}

// the PnP-RANSAC problem of a localisation as the chain runner queues it: solvePnPRansac(100, 1 px, 0.99) over the
// tracked sets, the frame's policy decided by the finishing kernel (VoChain)
svo_pnp_job pnp_job(svo_vo *v, const int *cnt_trk, uint64_t seed, int set = 0)
{
    svo_pnp_job q;
    q.obj = set ? v->trk3d_b : v->trk3d;
    q.img = set ? v->trk2d_b : v->trk2d;
    q.cap = v->cap;
    q.d_n = cnt_trk;
    q.K4[0] = v->prm.fx;
    q.K4[1] = v->prm.fy;
    q.K4[2] = v->prm.cx;
    q.K4[3] = v->prm.cy;
    q.iterations = 100;
    q.reproj_err = 1.0;
    q.confidence = 0.99;
    q.seed = seed;
    q.refine_iters = 20;
    q.inliers = set ? v->idx_b : v->idx;
    q.mask = nullptr;
    q.d_result = v->d_rec + set;
    q.chain = v->d_chain;
    q.cnt_trk = cnt_trk;
    return q;
}

// The pose ladder of the older visualOdometry::initSequence, src/bundleAdjust.cpp:462-480, on device point
// sets: (obj_f, img_f, cnt_f) = the tracked set after the F-matrix filter, (obj_s, img_s, cnt_s) = the
// status-filtered set ("retracking" without the filter gives exactly that: LK is deterministic).
//   rung 0  solvePnPRansac(100, 4.0, 0.99) on the filtered set
//   rung 1  < 20 inliers or tvec.x > 1000: the same on the status-filtered set
//   rung 2  < 10 inliers (or tvec.x > 1000 after rung 1): plain solvePnP on the set last used
// The record of the deciding solve is left in the context's pinned block (n_tracked = size of the set
// used; n_inliers = 0 when solvePnP had no solution); *ransac_inliers = the last RANSAC's count.
int ladder_pose(svo_ctx *ctx, const float *obj_f, const float *img_f, const int *cnt_f, const float *obj_s,
                const float *img_s, const int *cnt_s, int cap, const double *K4, uint64_t seed1, uint64_t seed2,
                int *idx_scratch, PnpRecord *d_rec, int *rung, int *ransac_inliers = nullptr)
{
    int rc;
    const PnpRecord *rec = reinterpret_cast<const PnpRecord *>(ctx->pinned);
    auto fetch = [&](const int *cnt) -> int {
        hipLaunchKernelGGL(store_count_kernel, dim3(1), dim3(1), 0, ctx->stream, cnt, &d_rec->n_tracked);
        SVO_HIP(hipMemcpyAsync(ctx->pinned, d_rec, sizeof(PnpRecord), hipMemcpyDeviceToHost, ctx->stream));
        return svo_wait(ctx);
    };
    const float *o3 = obj_f, *o2 = img_f;
    const int *cnt = cnt_f;
    *rung = 0;
    if ((rc = svo_launch_pnp_ransac(ctx, o3, o2, cap, cnt, K4, 100, 4.0, 0.99, seed1, 20, idx_scratch, nullptr, d_rec)) ||
        (rc = fetch(cnt)))
        return rc;
    bool plain = false;
    if (rec->n_inliers < 20 || rec->tvec[0] > 1000) {
        *rung = 1;
        o3 = obj_s;
        o2 = img_s;
        cnt = cnt_s;
        if ((rc = svo_launch_pnp_ransac(ctx, o3, o2, cap, cnt, K4, 100, 4.0, 0.99, seed2, 20, idx_scratch, nullptr,
                                        d_rec)) ||
            (rc = fetch(cnt)))
            return rc;
        plain = rec->n_inliers < 10 || rec->tvec[0] > 1000;
    }
    const int ninl = rec->n_inliers;
    if (ransac_inliers)
        *ransac_inliers = ninl;
    if (plain || ninl < 10) {  // "Skipping RANSAC all together": cv::solvePnP on everything that was tracked
        *rung = 2;
        if ((rc = svo_launch_solve_pnp(ctx, o3, o2, cap, cnt, K4, 20, idx_scratch, d_rec)) || (rc = fetch(cnt)))
            return rc;
    }
    return SVO_OK;
}

int stereo_triangulate(svo_vo *v, const svo_pyramid *left, const svo_pyramid *right, const double *Rt,
                       float *out2d, float *out3d, int *n_out)
{
    svo_pyramid *l = const_cast<svo_pyramid *>(left), *r = const_cast<svo_pyramid *>(right);
    return stereo_triangulate_batch(1, &v, &l, &r, &Rt, &out2d, &out3d, &n_out);
}

}  // namespace

extern "C" {

void svo_vo_default_params(svo_vo_params *p)
{
    if (!p)
        return;
    p->fx = 7.188560000000e+02;  // include/visualSLAM.h:82-87
    p->fy = 7.188560000000e+02;
    p->cx = 6.071928000000e+02;
    p->cy = 1.852157000000e+02;
    p->baseline = 0.54;  // include/visualSLAM.h:68
    p->grid_step = 30;   // src/triangulation.cpp:89
    p->anms_keep = 0;
    p->keyframe_min_inliers = 200;  // src/VisualSLAM.cpp:120
    p->f_thr_stereo = 3.0;          // src/tracking.cpp:34
    p->f_thr_temporal = 1.0;        // src/tracking.cpp:75
    p->seed = 0;
    p->policy = SVO_POLICY_SLAM;
    p->pnp_retry_below = 10;  // src/keyFrameManagement.cpp:85
    p->pnp_lost_below = 10;   // src/keyFrameManagement.cpp:89
}

int svo_vo_create(svo_ctx *ctx, const svo_vo_params *params, int width, int height, int channels, svo_vo **out)
{
    SVO_CHECK_ARG(ctx && params && out);
    SVO_CHECK_ARG(channels == 1 || channels == 3);
    SVO_CHECK_ARG(params->grid_step > 0 && params->keyframe_min_inliers >= 0);
    SVO_CHECK_ARG(params->policy == SVO_POLICY_SLAM || params->policy == SVO_POLICY_VO_LADDER);
    SVO_CHECK_ARG(params->pnp_retry_below >= 1 && params->pnp_lost_below >= 1);
    *out = nullptr;
    SVO_HIP(hipSetDevice(ctx->device));
    svo_vo *v = new svo_vo();
    v->ctx = ctx;
    v->prm = *params;
    v->w = width;
    v->h = height;
    v->c = channels;
    v->cap = grid_axis(width, params->grid_step) * grid_axis(height, params->grid_step);
    if (v->cap < 16)
        v->cap = 16;
    int rc = SVO_OK;
    const size_t n = (size_t)v->cap;
    if ((rc = svo_pyramid_create(ctx, width, height, channels, SVO_MAX_LEVELS, &v->pyr_ref)) ||
        (rc = svo_pyramid_create(ctx, width, height, channels, SVO_MAX_LEVELS, &v->pyr_cur)) ||
        // the right image is only ever the SECOND image of a tracking pass: no derivative levels
        (rc = svo_pyramid_create_ex(ctx, width, height, channels, SVO_MAX_LEVELS, false, &v->pyr_right)) ||
        (rc = svo_pyramid_create_ex(ctx, width, height, channels, SVO_MAX_LEVELS, false, &v->pyr_right2)) ||
        (rc = svo_pyramid_create(ctx, width, height, channels, SVO_MAX_LEVELS, &v->pyr_next)) ||
        (rc = dev_alloc(&v->d_chain, 1)) ||
        (rc = dev_alloc(&v->ref2d, n * 2)) || (rc = dev_alloc(&v->ref3d, n * 3)) ||
        (rc = dev_alloc(&v->trk2d, n * 2)) || (rc = dev_alloc(&v->trk3d, n * 3)) ||
        (rc = dev_alloc(&v->a2, n * 2)) || (rc = dev_alloc(&v->b2, n * 2)) || (rc = dev_alloc(&v->c2, n * 2)) ||
        (rc = dev_alloc(&v->d2, n * 2)) || (rc = dev_alloc(&v->a3, n * 3)) || (rc = dev_alloc(&v->b3, n * 3)) ||
        (rc = dev_alloc(&v->resp, n)) || (rc = dev_alloc(&v->status, n)) || (rc = dev_alloc(&v->mask, n)) ||
        (rc = dev_alloc(&v->kf_col, n * 3)) ||
        (rc = dev_alloc(&v->st2, n)) || (rc = dev_alloc(&v->idx, n)) || (rc = dev_alloc(&v->d_cnt, 16)) ||
        (rc = dev_alloc(&v->d_rec, 2)) || (rc = dev_alloc(&v->d_img, (size_t)width * height * channels)) ||
        (rc = dev_alloc(&v->grid_xy, n * 2)) ||
        (rc = svo_launch_grid(ctx, height, width, params->grid_step, v->grid_xy, (int)n))) {
        svo_vo_destroy(v);
        return rc;
    }
    if (hipHostMalloc(reinterpret_cast<void **>(&v->h_chain), sizeof(VoChain), hipHostMallocDefault) != hipSuccess) {
        svo_set_error("front-end: cannot allocate the pinned state block");
        svo_vo_destroy(v);
        return SVO_ERR_HIP;
    }
    for (int i = 0; i < 9; i++)
        v->R[i] = (i % 4) == 0;
    v->t[0] = v->t[1] = v->t[2] = 0;
    *out = v;
    return SVO_OK;
}

int svo_vo_destroy(svo_vo *v)
{
    if (!v)
        return SVO_OK;
    (void)hipSetDevice(v->ctx->device);
    (void)hipStreamSynchronize(v->ctx->stream);
    svo_pyramid_destroy(v->ctx, v->pyr_ref);
    svo_pyramid_destroy(v->ctx, v->pyr_cur);
    svo_pyramid_destroy(v->ctx, v->pyr_right);
    svo_pyramid_destroy(v->ctx, v->pyr_next);
    svo_pyramid_destroy(v->ctx, v->pyr_right2);
    for (void *sg : {(void *)v->sig_flt, (void *)v->sig_dec})
        if (sg)
            (void)hipFree(sg);
    for (hipStream_t st : {v->stream_b, v->stream_p})
        if (st) {
            (void)hipStreamSynchronize(st);
            (void)hipStreamDestroy(st);
        }
    for (hipEvent_t e : {v->ev_flt, v->ev_lk, v->ev_dec, v->ev_ref, v->ev_pyr[0], v->ev_pyr[1], v->ev_pyr[2], v->ev_pyr[3], v->ev_p1[0],
                         v->ev_p1[1], v->ev_p1[2], v->ev_p1[3], v->ev_p3[0], v->ev_p3[1], v->ev_p3[2], v->ev_p3[3], v->ev_e[0], v->ev_e[1],
                         v->ev_e[2], v->ev_e[3], v->ev_c[0], v->ev_c[1], v->ev_c[2], v->ev_c[3]})
        if (e)
            (void)hipEventDestroy(e);
    {
        svo_vo::StereoLane &L = v->lane;
        if (L.ctx) {
            (void)hipStreamSynchronize(L.ctx->stream);
            (void)svo_ctx_destroy(L.ctx);
        }
        void *sb[] = {L.a2,        L.b2,        L.c2,        L.d2,         L.x2,         L.resp,   L.status,   L.st2,      L.mask,
                      L.idx,       L.cnt,       v->h_x1[0],  v->h_x1[1],   v->h_xyz[0],  v->h_xyz[1], v->h_cnt, v->trk2d_b, v->trk3d_b,
                      v->idx_b,    v->a2k[0],   v->statusk[0], v->h_x1[2],  v->h_xyz[2], v->status_b, v->a2k[1],  v->a2k[2],
                      v->statusk[1], v->statusk[2], v->h_x2[0], v->h_x2[1], v->h_x2[2]};
        for (void *b : sb)
            if (b)
                (void)hipFree(b);
    }
    if (v->d_stamps)
        (void)hipFree(v->d_stamps);
    if (v->h_chain)
        (void)hipHostFree(v->h_chain);
    if (v->h_out)
        (void)hipHostFree(v->h_out);
    if (v->d_chain)
        (void)hipFree(v->d_chain);
    if (v->kf_col)
        (void)hipFree(v->kf_col);
    void *bufs[] = {v->ref2d, v->ref3d, v->trk2d, v->trk3d, v->a2,   v->b2,    v->c2,    v->d2,   v->a3,
                    v->b3,    v->resp,  v->status, v->mask, v->st2, v->idx,   v->d_cnt, v->d_rec, v->d_img,
                    v->grid_xy};
    for (void *b : bufs)
        if (b)
            (void)hipFree(b);
    delete v;
    return SVO_OK;
}

int svo_vo_init(svo_vo *v, const uint8_t *left, const uint8_t *right, int mem, int *n_points)
{
    SVO_CHECK_ARG(v && left && right);
    SVO_CHECK_ARG(mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE);
    int rc;
    v->frame = 0;
    for (int i = 0; i < 9; i++)
        v->R[i] = (i % 4) == 0;
    v->t[0] = v->t[1] = v->t[2] = 0;
    const uint8_t *d = stage_image(v, left, mem, &rc);
    if (rc || (rc = svo_build_pyramid_from_device(v->ctx, v->pyr_ref, d)))
        return rc;
    d = stage_image(v, right, mem, &rc);
    if (rc || (rc = svo_build_pyramid_from_device(v->ctx, v->pyr_right, d)))
        return rc;
    // identity [R|t]: the world cloud equals the camera-frame one bit for bit (x * 1 + y * 0 + z * 0 + 0 in
    // double), and the camera-frame cloud lands in b3 as at every later keyframe (svo_vo_get_keyframe_cloud)
    static const double I34[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    if ((rc = stereo_triangulate(v, v->pyr_ref, v->pyr_right, I34, v->ref2d, v->ref3d, &v->nref)))
        return rc;
    v->has_cur = false;
    if (n_points)
        *n_points = v->nref;
    return SVO_OK;
}

int svo_vo_localize(svo_vo *v, const uint8_t *left, int mem, double *R9, double *t3, int *n_inliers,
                    int *n_tracked)
{
    SVO_CHECK_ARG(v && left && R9 && t3);
    SVO_CHECK_ARG(mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE);
    svo_ctx *ctx = v->ctx;
    int rc;
    v->frame++;
    const int n = v->nref;
    if (n_inliers)
        *n_inliers = 0;
    if (n_tracked)
        *n_tracked = 0;
    const uint8_t *d = stage_image(v, left, mem, &rc);
    if (rc || (rc = svo_build_pyramid_from_device(ctx, v->pyr_cur, d)))
        return rc;
    v->has_cur = true;
    if (n < 5) {
        svo_set_error("tracking lost: %d reference points", n);
        return SVO_ERR_TRACKING_LOST;
    }
    // PyrLKtrackFrame2Frame (src/tracking.cpp:46-91)
    if ((rc = svo_launch_lk(ctx, v->pyr_ref, v->pyr_cur, v->ref2d, n, v->a2, v->status, nullptr, nullptr)))
        return rc;
    if ((rc = svo_launch_compact(ctx, v->status, n, nullptr, v->ref2d, 2, v->b2, v->a2, 2, v->c2, v->ref3d, 3, v->a3,
                                 v->d_cnt)))
        return rc;
    {
        // the F-RANSAC's finishing wave also compacts by its mask (src/tracking.cpp:77-88)
        const svo_compact_job by_mask = {v->mask, n, v->d_cnt, {v->c2, v->a3, nullptr}, {v->trk2d, v->trk3d, nullptr},
                                         {2, 3, 0}, v->d_cnt + 1};
        if ((rc = svo_launch_fransac(ctx, v->b2, v->c2, n, v->d_cnt, v->prm.f_thr_temporal, 0.99, 1000, stage_seed(v, 0),
                                     v->mask, nullptr, nullptr, nullptr, &by_mask)))
            return rc;
    }
    const double K4[4] = {v->prm.fx, v->prm.fy, v->prm.cx, v->prm.cy};
    const PnpRecord *rec = reinterpret_cast<const PnpRecord *>(ctx->pinned);
    if (v->prm.policy == SVO_POLICY_VO_LADDER) {
        // visualOdometry::initSequence, src/bundleAdjust.cpp:452-480 (see svo_vo_params.policy)
        int rung = 0;
        if ((rc = ladder_pose(ctx, v->trk3d, v->trk2d, v->d_cnt + 1, v->a3, v->c2, v->d_cnt, n, K4, stage_seed(v, 1),
                              stage_seed(v, 2), v->idx, v->d_rec, &rung, &v->ladder_ransac_inliers)))
            return rc;
        if (rung >= 1) {  // the set the pose was computed from is the tracked set
            std::swap(v->trk2d, v->c2);
            std::swap(v->trk3d, v->a3);
        }
        v->ntrk = rec->n_tracked;
        if (n_inliers)
            *n_inliers = rung == 2 ? v->ladder_ransac_inliers : rec->n_inliers;
        if (n_tracked)
            *n_tracked = rec->n_tracked;
        if (rec->n_inliers == 0) {  // upstream: cv::Exception out of solvePnP (too few / planar points)
            svo_set_error("tracking lost at frame %d: solvePnP has no solution for %d points", v->frame, rec->n_tracked);
            return SVO_ERR_TRACKING_LOST;
        }
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++)
                R9[3 * i + j] = rec->R[3 * j + i];
        for (int i = 0; i < 3; i++)
            t3[i] = -(R9[3 * i] * rec->tvec[0] + R9[3 * i + 1] * rec->tvec[1] + R9[3 * i + 2] * rec->tvec[2]);
        return SVO_OK;
    }
    // solvePnPRansac (src/keyFrameManagement.cpp:84), retry (:85-92)
    for (int attempt = 0; attempt < 2; attempt++) {
        if ((rc = svo_launch_pnp_ransac(ctx, v->trk3d, v->trk2d, n, v->d_cnt + 1, K4, 100, attempt ? 8.0 : 1.0,
                                        attempt ? 0.98 : 0.99, stage_seed(v, attempt ? 2 : 1), 20, v->idx, nullptr,
                                        v->d_rec)))
            return rc;
        hipLaunchKernelGGL(store_count_kernel, dim3(1), dim3(1), 0, ctx->stream, v->d_cnt + 1, &v->d_rec->n_tracked);
        SVO_HIP(hipMemcpyAsync(ctx->pinned, v->d_rec, sizeof(PnpRecord), hipMemcpyDeviceToHost, ctx->stream));
        if ((rc = svo_wait(ctx)))
            return rc;
        if (rec->n_inliers >= (attempt ? v->prm.pnp_lost_below : v->prm.pnp_retry_below))
            break;
    }
    v->ntrk = rec->n_tracked;
    if (n_inliers)
        *n_inliers = rec->n_inliers;
    if (n_tracked)
        *n_tracked = rec->n_tracked;
    if (rec->n_inliers < v->prm.pnp_lost_below) {
        svo_set_error("tracking lost at frame %d: %d PnP inliers", v->frame, rec->n_inliers);
        return SVO_ERR_TRACKING_LOST;
    }
    // Rodrigues; R = R^T; t = -R * tvec (src/VisualSLAM.cpp:70-74)
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
            R9[3 * i + j] = rec->R[3 * j + i];
    for (int i = 0; i < 3; i++)
        t3[i] = -(R9[3 * i] * rec->tvec[0] + R9[3 * i + 1] * rec->tvec[1] + R9[3 * i + 2] * rec->tvec[2]);
    return SVO_OK;
}

int svo_vo_update(svo_vo *v, const uint8_t *right, int mem, const double *R9, const double *t3, int n_inliers,
                  int force_keyframe, int *was_keyframe)
{
    SVO_CHECK_ARG(v && R9 && t3);
    SVO_CHECK_ARG(mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE);
    if (!v->has_cur) {
        svo_set_error("svo_vo_update without a preceding svo_vo_localize");
        return SVO_ERR_STATE;
    }
    memcpy(v->R, R9, sizeof(v->R));
    memcpy(v->t, t3, sizeof(v->t));
    // src/VisualSLAM.cpp:120; the older ladder re-triangulates on every frame (src/bundleAdjust.cpp:517-519)
    const bool kf = n_inliers < v->prm.keyframe_min_inliers || force_keyframe || v->prm.policy == SVO_POLICY_VO_LADDER;
    if (kf) {
        SVO_CHECK_ARG(right != nullptr);
        int rc;
        const uint8_t *d = stage_image(v, right, mem, &rc);
        if (rc || (rc = svo_build_pyramid_from_device(v->ctx, v->pyr_right, d)))
            return rc;
        double Rt[12];
        for (int i = 0; i < 3; i++) {
            Rt[4 * i] = R9[3 * i];
            Rt[4 * i + 1] = R9[3 * i + 1];
            Rt[4 * i + 2] = R9[3 * i + 2];
            Rt[4 * i + 3] = t3[i];
        }
        // insertKeyFrames (src/keyFrameManagement.cpp:9-31): re-triangulate at the current frame
        if ((rc = stereo_triangulate(v, v->pyr_cur, v->pyr_right, Rt, v->ref2d, v->ref3d, &v->nref)))
            return rc;
    } else {  // src/VisualSLAM.cpp:143-146: carry the tracked sets forward
        std::swap(v->ref2d, v->trk2d);
        std::swap(v->ref3d, v->trk3d);
        v->nref = v->ntrk;
    }
    std::swap(v->pyr_ref, v->pyr_cur);  // referenceImg = currentImage (src/VisualSLAM.cpp:151)
    v->has_cur = false;
    if (was_keyframe)
        *was_keyframe = kf ? 1 : 0;
    return SVO_OK;
}

int svo_vo_track(svo_vo *v, const uint8_t *left, const uint8_t *right, int mem, int force_keyframe, double *R9,
                 double *t3, int *n_inliers, int *was_keyframe, int *n_tracked)
{
    int ninl = 0;
    int rc = svo_vo_localize(v, left, mem, R9, t3, &ninl, n_tracked);
    if (n_inliers)
        *n_inliers = ninl;
    if (rc)
        return rc;
    return svo_vo_update(v, right, mem, R9, t3, ninl, force_keyframe, was_keyframe);
}

// ---- the chain runner --------------------------------------------------------------------------------------------
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
// pipeline (one chunk, device images): three HIP streams, see svo_vo and chain_enqueue.  The PnP of frame t runs on a
// stream of its own while the context's stream builds the pyramids of frame t+1 and tracks into them from the points
// frame t kept -- which is what frame t+1 does unless frame t turns out to be a keyframe, in which case a second tracking
// launch (gated on the keyframe flag) redoes it from the new keyframe's points; the stereo path of every frame runs a
// frame ahead on a third stream.
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
    for (int a = 0; a < k; a++) {
        LkJob &q = lk[a];
        q.prev = prev[a]->dev;
        q.next = next[a]->dev;
        q.dprev = prev[a]->dbase;
        q.prev_pts = pts[a];
        q.n_cap = vs[a]->cap;
        q.d_n = d_n[a];
        q.next_pts = vs[a]->a2;
        q.status = vs[a]->status;
        q.err = nullptr;
        q.min_eig = nullptr;
        q.gate = gates[a];
    }
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
        const int *run = &v->d_chain->run;
        if (kf_slot >= 0) {
            c1[a] = {st_par ? v->status_b : v->status, v->cap, &v->d_chain->nref, {v->ref2d, v->a2, nullptr},
                     {v->b2, v->c2, nullptr}, {2, 2, 0}, v->d_cnt, run};
            c1[a].alt_sel = &v->d_chain->kf;
            c1[a].alt_mask = v->statusk[kbuf];
            c1[a].alt_in[0] = v->h_x1[kf_slot];
            c1[a].alt_in[1] = v->a2k[kbuf];
            c1[a].alt_d_n = v->h_cnt + kf_slot;
            c2[a] = {v->mask, v->cap, v->d_cnt, {v->c2, nullptr, nullptr}, {set ? v->trk2d_b : v->trk2d, nullptr, nullptr},
                     {2, 0, 0}, v->d_cnt + (set ? 9 : 1)};
        } else {
            c1[a] = {v->status, v->cap, &v->d_chain->nref, {v->ref2d, v->a2, v->ref3d}, {v->b2, v->c2, v->a3}, {2, 2, 3},
                     v->d_cnt, run};
            c2[a] = {v->mask, v->cap, v->d_cnt, {v->c2, v->a3, nullptr},
                     {set ? v->trk2d_b : v->trk2d, set ? v->trk3d_b : v->trk3d, nullptr}, {2, 3, 0}, v->d_cnt + (set ? 9 : 1)};
        }
        svo_fransac_job &q = fj[a];
        q.p1 = v->b2;
        q.p2 = v->c2;
        q.cap = v->cap;
        q.d_n = v->d_cnt;
        q.threshold = v->prm.f_thr_temporal;
        q.confidence = 0.99;
        q.max_iters = 1000;
        q.seed = stage_seed(v, 0);
        q.mask = v->mask;
        q.d_F = nullptr;
        q.d_count = nullptr;
        q.d_iters = nullptr;
        q.then_compact = &c2[a];  // the mask compaction rides with the F-RANSAC
        q.gate = run;
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
            {3, 0, 0}, v->d_cnt + 10, run};
    c[0].alt_sel = &v->d_chain->kf;  // still the previous frame's decision
    c[0].alt_mask = v->statusk[kbuf];
    c[1] = {v->mask, v->cap, v->d_cnt + 10, {v->a3, nullptr, nullptr}, {set ? v->trk3d_b : v->trk3d, nullptr, nullptr},
            {3, 0, 0}, v->d_cnt + 11, run};
    int rc;
    if ((rc = svo_launch_compact_batch(ctx, 1, &c[0])) || (rc = svo_launch_compact_batch(ctx, 1, &c[1])))
        return rc;
    return SVO_OK;
}

static int chain_pnp(svo_ctx *ctx, int k, svo_vo *const *vs, int set = 0, bool split = false)
{
    svo_pnp_job pj[SVO_LK_MAX_JOBS];
    for (int a = 0; a < k; a++)
        pj[a] = pnp_job(vs[a], vs[a]->d_cnt + (set ? 9 : 1), stage_seed(vs[a], 1), set);
    return svo_launch_pnp_ransac_batch(ctx, k, pj, split);
}

// the refinement a split chain_pnp left undone, for the frame if it is a keyframe / if it is none
static int chain_pnp_refine(svo_ctx *ctx, svo_vo *const *vs, int set, bool keyframes)
{
    const svo_pnp_job pj = pnp_job(vs[0], vs[0]->d_cnt + (set ? 9 : 1), stage_seed(vs[0], 1), set);
    return svo_launch_pnp_refine(ctx, 1, &pj, keyframes);
}

// Queue frames [0, n) of k chunks that share a context (lock step: every stage one set of launches for all of them;
// chunks may differ in length).  pipeline: k == 1, device images.
static int chain_enqueue(ChainRun *const *runs, int k, bool pipeline)
{
    svo_vo *v0 = runs[0]->v;
    svo_ctx *ctx = v0->ctx;
    int n_max = 0, rc;
    for (int a = 0; a < k; a++)
        n_max = runs[a]->n_frames > n_max ? runs[a]->n_frames : n_max;
    if (n_max == 0)
        return SVO_OK;
    auto upload = [&](svo_vo *v, const uint8_t *img, int mem) -> const uint8_t * {  // host images: the one staging buffer
        return stage_image(v, img, mem, &rc);
    };
    svo_vo *vs[SVO_LK_MAX_JOBS];
    svo_pyramid *prevs[SVO_LK_MAX_JOBS], *nexts[SVO_LK_MAX_JOBS];
    const float *pts[SVO_LK_MAX_JOBS];
    const int *dn[SVO_LK_MAX_JOBS], *gates[SVO_LK_MAX_JOBS];
    // the pyramids of one frame of the active chunks: the left images and, in the same set of launches, the right ones
    auto build = [&](int na, svo_vo *const *va, svo_pyramid *const *lp, svo_pyramid *const *rp, const uint8_t *const *li,
                     const uint8_t *const *ri, int mem) -> int {
        if (mem == SVO_MEM_HOST) {  // one chunk, one staging buffer: upload + build, twice
            const int *g = &va[0]->d_chain->run;
            const uint8_t *d = upload(va[0], li[0], mem);
            if (rc || (rc = svo_build_pyramids_from_device(ctx, 1, &lp[0], &d, &g)))
                return rc;
            d = upload(va[0], ri[0], mem);
            if (rc || (rc = svo_build_pyramids_from_device(ctx, 1, &rp[0], &d, &g)))
                return rc;
            return SVO_OK;
        }
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
    };
    if (pipeline) {
        // Four streams (see svo_vo).  Nothing on A waits for the frame's decision: after the filters of frame f it runs
        // BOTH tracking passes into frame f+1 -- from the tracked set and from the 2-D points the stereo path of f has
        // left -- as one launch (the launch lasts as long as its slowest keypoint: two passes cost less than two
        // launches), and the filters of f+1 take the status bytes and points of the one the decision points to (the
        // compaction selects by the keyframe flag on the device).  B: PnP hypotheses, the decision, then a keyframe's
        // refinement and the hand-over of its sets (the 2-D points become the reference set, the cloud is placed with
        // the refined pose), which A waits for before the next filters; any other frame's refinement after that.
        // C: the stereo path of EVERY frame, two frames ahead, started when A's tracking launch has ended (its own
        // tracking pass then runs beside A's filters instead of beside A's launch).  D: the pyramids, two frames ahead.
        static const bool dbg = getenv("SVO_CHAIN_DEBUG") != nullptr;
        double us_cat[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // host time by category (debug): see the print below
        auto tick = [&]() { return dbg ? std::chrono::steady_clock::now() : std::chrono::steady_clock::time_point(); };
        auto tock = [&](int cat, std::chrono::steady_clock::time_point t0) {
            if (dbg)
                us_cat[cat] += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        };
        ChainRun &r = *runs[0];
        svo_vo *v = r.v;
        hipStream_t sA = ctx->stream, sB = v->stream_b, sC = v->lane.ctx->stream, sD = v->stream_p;
        hipStream_t sE = sD;  // the keyframe passes share the pyramids' stream: a fifth busy queue costs more than it brings
        // debug: device time stamps between the stages (8 per frame: A0 before filters, A1 after, A2 after the tracking
        // launch, B0 before hypotheses, B1 decided, B2 handed over, C0 / C1 around the stereo path)
        // SVO_PIPE_MEMOPS=1: the two hand-overs as stream memory operations instead of events.  Measured: B starts 5 us after
        // the filters instead of 11-17, frames/s unchanged (3 071 against 3 084) -- the hops are not what limits a frame; the
        // API is marked beta, so events stay the default.
        static const bool memops = getenv("SVO_PIPE_MEMOPS") ? atoi(getenv("SVO_PIPE_MEMOPS")) != 0 : false;
        static const bool stamps_env = getenv("SVO_CHAIN_STAMPS") != nullptr;
        const bool stamps = stamps_env || v->stamps_on;
        const int max_stamp_frames = 4096;
        if (stamps && !v->d_stamps)
            SVO_HIP(hipMalloc(reinterpret_cast<void **>(&v->d_stamps), sizeof(unsigned long long) * 8 * max_stamp_frames));
        unsigned long long *d_stamps = v->d_stamps;
        auto stamp = [&](hipStream_t st, int frame, int slot) {
            if (stamps && frame < max_stamp_frames)
                hipLaunchKernelGGL(stamp_kernel, dim3(1), dim3(1), 0, st, d_stamps + 8 * frame + slot);
        };
        svo_pyramid *ref = v->pyr_ref, *cur = v->pyr_cur, *nxt = v->pyr_next;
        svo_pyramid *right[2] = {v->pyr_right, v->pyr_right2};
        const int *run = &v->d_chain->run;
        vs[0] = v;
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
            if ((rc = build(1, vs, &left, &rp, &li, &ri, r.mem)))
                return rc;
            SVO_HIP(hipEventRecord(v->ev_pyr[g & 3], sD));
            return SVO_OK;
        };
        // the stereo path of frame g on C, from the pyramids D has built
        auto stereo = [&](int g, svo_pyramid *left) -> int {
            SVO_HIP(hipStreamWaitEvent(sC, v->ev_pyr[g & 3], 0));
            if ((rc = stereo_part1_spec(v, v->lane, left, right[g & 1], frame0 + g + 1, g % 3)))
                return rc;
            SVO_HIP(hipEventRecord(v->ev_c[g & 3], sC));
            return SVO_OK;
        };
        // ... and its triangulation, on D
        auto triangulate = [&](int g) -> int {
            SVO_HIP(hipStreamWaitEvent(sD, v->ev_c[g & 3], 0));
            {
                OnStream on(ctx, sD);
                if ((rc = stereo_tri_spec(v, g % 3)))
                    return rc;
            }
            SVO_HIP(hipEventRecord(v->ev_p1[g & 3], sD));
            return SVO_OK;
        };
        // E: the tracking pass into frame g from the 2-D points the stereo path of frame g-1 has left -- what frame g starts
        // from if g-1 turns out to be a keyframe.  Nothing in it depends on a decision or a tracked set: it runs as soon as
        // that stereo path and the pyramids of g exist, a frame and a half before the filters that may read it.
        auto kf_pass = [&](int g, svo_pyramid *from, svo_pyramid *into) -> int {
            SVO_HIP(hipStreamWaitEvent(sE, v->ev_c[(g - 1) & 3], 0));  // the 2-D points of that stereo path
            SVO_HIP(hipStreamWaitEvent(sE, v->ev_pyr[g & 3], 0));
            LkJob q;
            q.prev = from->dev;
            q.next = into->dev;
            q.dprev = from->dbase;
            q.prev_pts = v->h_x1[(g - 1) % 3];
            q.n_cap = v->cap;
            q.d_n = v->h_cnt + (g - 1) % 3;
            q.next_pts = v->a2k[g % 3];
            q.status = v->statusk[g % 3];
            q.err = nullptr;
            q.min_eig = nullptr;
            q.gate = run;
            {
                OnStream on(ctx, sE);
                if ((rc = svo_launch_lk_batch(ctx, 1, &q, from)))
                    return rc;
            }
            SVO_HIP(hipEventRecord(v->ev_e[g & 3], sE));
            return SVO_OK;
        };
        // prologue: the chain state is on its way (chain_prepare, on A); the pyramids of frames 0 and 1, the tracking
        // pass into frame 0 from the reference set, the stereo paths of frames 0 and 1, the keyframe pass into frame 1
        SVO_HIP(hipEventRecord(v->ev_flt, sA));
        SVO_HIP(hipStreamWaitEvent(sD, v->ev_flt, 0));
        if ((rc = pyramids(0, cur)) || (nf > 1 && (rc = pyramids(1, nxt))))
            return rc;
        {
            SVO_HIP(hipStreamWaitEvent(sA, v->ev_pyr[0], 0));
            pts[0] = v->ref2d;
            dn[0] = &v->d_chain->nref;
            gates[0] = run;
            if ((rc = chain_lk(ctx, 1, vs, &ref, &cur, pts, dn, gates)))
                return rc;
            if ((rc = stereo(0, cur)) || (nf > 1 && (rc = stereo(1, nxt))) || (rc = triangulate(0)) ||
                (nf > 1 && (rc = kf_pass(1, cur, nxt))))
                return rc;
        }
        if (nf > 1)
            SVO_HIP(hipStreamWaitEvent(sA, v->ev_pyr[1], 0));  // the first tracking launch's target
        for (int f = 0; f < nf; f++) {
            v->frame++;
            const int set = f & 1, slot = f % 3;
            const bool more = f + 1 < nf;
            auto t0 = tick();
            stamp(sA, f, 0);
            // the 2-D half of the filters; the previous frame a keyframe: from the sets of the pass that started at its points
            if ((rc = chain_filters(ctx, 1, vs, set, (f + 2) % 3, f & 1, f % 3)))
                return rc;
            const uint32_t tick_no = ++v->sig_n;  // this frame's value of the two signals
            if (memops)
                SVO_HIP(hipStreamWriteValue32(sA, v->sig_flt, tick_no, 0));
            SVO_HIP(hipEventRecord(v->ev_flt, sA));
            stamp(sA, f, 1);
            tock(0, t0);
            t0 = tick();
            // B: the 3-D column of the filters, hypotheses, the decision (all A waits for); then a keyframe is refined and
            // its sets handed over; any other frame is refined after that.  (In order on B: the next frame's 3-D column
            // follows the hand-over it reads, its hypotheses follow this frame's refinement, which reads the workspace
            // they are written to.)
            if (memops)
                SVO_HIP(hipStreamWaitValue32(sB, v->sig_flt, tick_no, hipStreamWaitValueGte, 0xffffffffu));
            else
                SVO_HIP(hipStreamWaitEvent(sB, v->ev_flt, 0));
            {
                OnStream on(ctx, sB);
                stamp(sB, f, 3);
                if ((rc = chain_filters_3d(ctx, v, set, f & 1, f % 3)) || (rc = chain_pnp(ctx, 1, vs, set, true)))
                    return rc;
                if (memops)
                    SVO_HIP(hipStreamWriteValue32(sB, v->sig_dec, tick_no, 0));
                else
                    SVO_HIP(hipEventRecord(v->ev_dec, sB));
                stamp(sB, f, 4);
                SVO_HIP(hipStreamWaitEvent(sB, v->ev_p1[f & 3], 0));  // the stereo path of this frame: long done
                if ((rc = chain_pnp_refine(ctx, vs, set, true)) || (rc = stereo_part2_spec(v, cur, slot, 3)))
                    return rc;
                stamp(sB, f, 5);
                SVO_HIP(hipEventRecord(v->ev_p3[f & 3], sB));
                if ((rc = chain_pnp_refine(ctx, vs, set, false)))
                    return rc;
            }
            tock(1, t0);
            t0 = tick();
            // D: the pyramids of frame f+2 into the buffer of frame f-1, whose last readers were the tracking launch of
            // the previous iteration (before these filters on A), the stereo path of frame f-1 (C is in order: frame f's
            // is done) and the colours of keyframe f-1 (its hand-over on B); the right pyramid it overwrites is the one
            // the stereo path of frame f has read
            if (more) {
                SVO_HIP(hipStreamWaitEvent(sD, v->ev_flt, 0));
                SVO_HIP(hipStreamWaitEvent(sD, v->ev_c[f & 3], 0));
                if (f > 0)  // ... and the hand-over of keyframe f-2 (B is in order), whose cloud's buffer the triangulation below writes
                    SVO_HIP(hipStreamWaitEvent(sD, v->ev_p3[(f - 1) & 3], 0));
                if (f + 2 < nf && (rc = pyramids(f + 2, ref)))
                    return rc;
                if ((rc = triangulate(f + 1)))  // the stereo path of the next frame ends here (its 2-D part is long done)
                    return rc;
            }
            tock(2, t0);
            t0 = tick();
            if (more) {  // A: the tracking pass into frame f+1 from the tracked set
                pts[0] = set ? v->trk2d_b : v->trk2d;
                dn[0] = v->d_cnt + (set ? 9 : 1);
                gates[0] = run;
                LkJob q;
                q.prev = cur->dev;
                q.next = nxt->dev;
                q.dprev = cur->dbase;
                q.prev_pts = pts[0];
                q.n_cap = v->cap;
                q.d_n = dn[0];
                q.next_pts = v->a2;
                q.status = (f + 1) & 1 ? v->status_b : v->status;
                q.err = nullptr;
                q.min_eig = nullptr;
                q.gate = run;
                if ((rc = svo_launch_lk_batch(ctx, 1, &q, cur)))
                    return rc;
                stamp(sA, f, 2);
                SVO_HIP(hipEventRecord(v->ev_lk, sA));
                tock(3, t0);
                t0 = tick();
                // C: the stereo path of frame f+2 once this launch has ended.  It writes the hand-over set of frame f-1,
                // whose readers were the previous iteration's launch and that frame's hand-over on B.
                if (f + 2 < nf) {
                    SVO_HIP(hipStreamWaitEvent(sC, v->ev_lk, 0));
                    if (f > 0)
                        SVO_HIP(hipStreamWaitEvent(sC, v->ev_p3[(f - 1) & 3], 0));
                    stamp(sC, f, 6);
                    if ((rc = stereo(f + 2, ref)))  // `ref`: where D has just been told to build frame f+2
                        return rc;
                    stamp(sC, f, 7);
                    // E: the keyframe pass from frame f+1 into frame f+2, when A's launch has ended too.  Its output
                    // buffer (target % 3) was last read by the filters of frame f-1 on A and B, before the decision A
                    // waited for at the end of the previous iteration.
                    SVO_HIP(hipStreamWaitEvent(sE, v->ev_lk, 0));
                    if ((rc = kf_pass(f + 2, nxt, ref)))
                        return rc;
                }
                tock(4, t0);
            }
            // What the next iteration needs of the streams that run ahead is waited for HERE, before the wait for the
            // decision: every wait is a barrier packet of ~7 us on the stream, and while B decides this stream is idle
            // anyway -- after the decision nothing but the filters' launches is left.
            if (f + 2 < nf)
                SVO_HIP(hipStreamWaitEvent(sA, v->ev_pyr[(f + 2) & 3], 0));  // the next tracking launch's target
            if (more)
                SVO_HIP(hipStreamWaitEvent(sA, v->ev_e[(f + 1) & 3], 0));    // the keyframe pass the next filters may read
            if (memops)  // the next filters: the keyframe flag, a plain frame's 2-D set
                SVO_HIP(hipStreamWaitValue32(sA, v->sig_dec, tick_no, hipStreamWaitValueGte, 0xffffffffu));
            else
                SVO_HIP(hipStreamWaitEvent(sA, v->ev_dec, 0));
            svo_pyramid *t = ref;  // referenceImg = currentImage (src/VisualSLAM.cpp:151)
            ref = cur;
            cur = nxt;
            nxt = t;
        }
        // the last frame's refinement runs on B: the caller's wait on A covers it
        SVO_HIP(hipEventRecord(v->ev_ref, sB));
        SVO_HIP(hipStreamWaitEvent(sA, v->ev_ref, 0));
        if (dbg)
            fprintf(stderr, "[svo chain] host us per frame: filters + record %.1f, B %.1f, D %.1f, tracking launch on A %.1f, C %.1f\n",
                    us_cat[0] / nf, us_cat[1] / nf, us_cat[2] / nf, us_cat[3] / nf, us_cat[4] / nf);
        if (stamps && nf > 40) {  // wait, read, keep (and print, with the environment switch) the mean intervals over the middle of the run
            SVO_HIP(hipStreamSynchronize(sA));
            SVO_HIP(hipStreamSynchronize(sC));
            const int n = nf < max_stamp_frames ? nf : max_stamp_frames;
            std::vector<unsigned long long> h((size_t)8 * n);
            SVO_HIP(hipMemcpy(h.data(), d_stamps, h.size() * sizeof(h[0]), hipMemcpyDeviceToHost));
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
            if (stamps_env)
                fprintf(stderr, "[svo chain] device us per frame (stamps): cycle %.1f = filters %.1f + tracking launch %.1f + wait for B %.1f | "
                                "B starts %.1f after the filters, PnP to decision %.1f, refine + hand-over of a keyframe %.1f | C starts %.1f "
                                "after the launch, stereo path %.1f\n", cyc / m, filt / m, lk / m, a_wait / m, b_lag / m, pnp / m, hand / m,
                        c_lag / m, c_len / m);
        }
        return SVO_OK;
    }
    // lock step on one stream
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
        if ((rc = build(na, vs, nexts, rp, li, ri, SVO_MEM_DEVICE)))
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
    int *cnt = v->d_cnt + (r.halt_set ? 9 : 1);
    const double K4[4] = {v->prm.fx, v->prm.fy, v->prm.cx, v->prm.cy};
    const PnpRecord *rec = reinterpret_cast<const PnpRecord *>(ctx->pinned);
    if ((rc = svo_launch_pnp_ransac(ctx, v->trk3d, v->trk2d, v->cap, cnt, K4, 100, 8.0, 0.98, stage_seed(v, 2), 20, v->idx,
                                    nullptr, v->d_rec)))
        return rc;
    hipLaunchKernelGGL(store_count_kernel, dim3(1), dim3(1), 0, ctx->stream, cnt, &v->d_rec->n_tracked);
    SVO_HIP(hipMemcpyAsync(ctx->pinned, v->d_rec, sizeof(PnpRecord), hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = svo_wait(ctx)))
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
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
            R9[3 * i + j] = rec->R[3 * j + i];
    for (int i = 0; i < 3; i++)
        t3[i] = -(R9[3 * i] * rec->tvec[0] + R9[3 * i + 1] * rec->tvec[1] + R9[3 * i + 2] * rec->tvec[2]);
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
            if (v->nref < 5) {
                svo_set_error("tracking lost: %d reference points", v->nref);
                r.rc = SVO_ERR_TRACKING_LOST;
                break;
            }
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
        pipeline = 0;  // host images go through one staging buffer; keep them strictly in order
    if (pipeline && !v->pipe_ready) {
        // The pipeline's streams exist only once pipelining is asked for.  The PnP stream is in the high-priority class:
        // HIP keeps a separate pool of hardware queues per priority class, so the streams of a chunk never land on one
        // queue (with all in the default class the runtime was seen to put two of them on the same queue, which
        // serialises the overlap away), and creating it does not disturb the stream -> queue assignment of serial chunks
        // running side by side.
        int rc, prio_lo = 0, prio_hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
        if (!v->stream_b)
            SVO_HIP(hipStreamCreateWithPriority(&v->stream_b, hipStreamNonBlocking, prio_hi));
        if (!v->stream_p)
            SVO_HIP(hipStreamCreateWithFlags(&v->stream_p, hipStreamNonBlocking));
        const size_t n = (size_t)v->cap;
        svo_vo::StereoLane &L = v->lane;
        if (!L.ctx && (rc = svo_ctx_create(v->ctx->device, &L.ctx)))
            return rc;
        if ((!L.a2 && (rc = dev_alloc(&L.a2, n * 2))) || (!L.b2 && (rc = dev_alloc(&L.b2, n * 2))) ||
            (!L.c2 && (rc = dev_alloc(&L.c2, n * 2))) || (!L.d2 && (rc = dev_alloc(&L.d2, n * 2))) ||
            (!L.x2 && (rc = dev_alloc(&L.x2, n * 2))) || (!L.resp && (rc = dev_alloc(&L.resp, n))) ||
            (!L.status && (rc = dev_alloc(&L.status, n))) || (!L.st2 && (rc = dev_alloc(&L.st2, n))) ||
            (!L.mask && (rc = dev_alloc(&L.mask, n))) || (!L.idx && (rc = dev_alloc(&L.idx, n))) ||
            (!L.cnt && (rc = dev_alloc(&L.cnt, 16))))
            return rc;
        for (int k = 0; k < 3; k++)
            if ((!v->h_x2[k] && (rc = dev_alloc(&v->h_x2[k], n * 2))) || (!v->h_x1[k] && (rc = dev_alloc(&v->h_x1[k], n * 2))) || (!v->h_xyz[k] && (rc = dev_alloc(&v->h_xyz[k], n * 3))))
                return rc;
        if ((!v->h_cnt && (rc = dev_alloc(&v->h_cnt, 16))) || (!v->trk2d_b && (rc = dev_alloc(&v->trk2d_b, n * 2))) ||
            (!v->trk3d_b && (rc = dev_alloc(&v->trk3d_b, n * 3))) || (!v->idx_b && (rc = dev_alloc(&v->idx_b, n))) ||
            (!v->status_b && (rc = dev_alloc(&v->status_b, n))))
            return rc;
        for (int k = 0; k < 3; k++)
            if ((!v->a2k[k] && (rc = dev_alloc(&v->a2k[k], n * 2))) || (!v->statusk[k] && (rc = dev_alloc(&v->statusk[k], n))))
                return rc;
        for (hipEvent_t *e : {&v->ev_flt, &v->ev_lk, &v->ev_dec, &v->ev_ref, &v->ev_pyr[0], &v->ev_pyr[1], &v->ev_pyr[2], &v->ev_pyr[3],
                              &v->ev_p1[0], &v->ev_p1[1], &v->ev_p1[2], &v->ev_p1[3], &v->ev_p3[0], &v->ev_p3[1], &v->ev_p3[2],
                              &v->ev_p3[3], &v->ev_e[0], &v->ev_e[1], &v->ev_e[2], &v->ev_e[3], &v->ev_c[0], &v->ev_c[1],
                              &v->ev_c[2], &v->ev_c[3]})
            if (!*e)
                SVO_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
        if (!v->sig_flt) {
            SVO_HIP(hipExtMallocWithFlags(reinterpret_cast<void **>(&v->sig_flt), 8, hipMallocSignalMemory));
            SVO_HIP(hipExtMallocWithFlags(reinterpret_cast<void **>(&v->sig_dec), 8, hipMallocSignalMemory));
            SVO_HIP(hipMemset(v->sig_flt, 0, 8));
            SVO_HIP(hipMemset(v->sig_dec, 0, 8));
        }
        v->pipe_ready = true;
    }
    if (v->nref < 5) {
        svo_set_error("tracking lost: %d reference points", v->nref);
        return SVO_ERR_TRACKING_LOST;
    }
    ChainRun r;
    r.v = v;
    r.lefts = lefts;
    r.rights = rights;
    r.n_frames = n_frames;
    r.mem = mem;
    r.R_out = R_out;
    r.t_out = t_out;
    r.inliers_out = inliers_out;
    r.tracked_out = tracked_out;
    r.keyframe_out = keyframe_out;
    ChainRun *one = &r;
    int rc = chain_run(&one, 1, pipeline != 0);
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
            for (int i = 0; i < 9; i++)
                v->R[i] = (i % 4) == 0;
            v->t[0] = v->t[1] = v->t[2] = 0;
            v->has_cur = false;
            vs[ni] = v;
            pl[ni] = v->pyr_ref;
            pr[ni] = v->pyr_right;
            il[ni] = j->init_left;
            ir[ni] = j->init_right;
            static const double I34[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
            Rts[ni] = I34;  // as svo_vo_init
            o2d[ni] = v->ref2d;
            o3d[ni] = v->ref3d;
            nout[ni] = &v->nref;
            ni++;
        }
        if (ni > 0 && jobs[0]->mem == SVO_MEM_HOST) {
            // host images: the initialisation's frames go through the upload ring's memory on the group's own stream (the
            // run's first uploads are ordered behind what this stream has queued, chain_enqueue)
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
        if (j->vo->nref < 5) {
            svo_set_error("tracking lost: %d reference points", j->vo->nref);
            j->rc = SVO_ERR_TRACKING_LOST;
            continue;
        }
        ChainRun &r = runs[nr];
        r.v = j->vo;
        r.lefts = j->lefts;
        r.rights = j->rights;
        r.n_frames = j->n_frames;
        r.mem = j->mem;
        r.R_out = j->R_out;
        r.t_out = j->t_out;
        r.inliers_out = j->inliers_out;
        r.tracked_out = j->tracked_out;
        r.keyframe_out = j->keyframe_out;
        rp[nr++] = &r;
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

int svo_vo_get_reference(svo_vo *v, float *ref2d, float *ref3d, int cap, int *n, int mem)
{
    SVO_CHECK_ARG(v && n);
    *n = v->nref;
    if (cap < v->nref) {
        svo_set_error("reference set has %d points, capacity %d", v->nref, cap);
        return SVO_ERR_CAPACITY;
    }
    const hipMemcpyKind kind = mem == SVO_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (ref2d)
        SVO_HIP(hipMemcpyAsync(ref2d, v->ref2d, (size_t)v->nref * 8, kind, v->ctx->stream));
    if (ref3d)
        SVO_HIP(hipMemcpyAsync(ref3d, v->ref3d, (size_t)v->nref * 12, kind, v->ctx->stream));
    SVO_HIP(hipStreamSynchronize(v->ctx->stream));
    return SVO_OK;
}

int svo_pnp_ladder(svo_ctx *ctx, const float *obj_f, const float *img_f, int n_f, const float *obj_s, const float *img_s,
                   int n_s, const double *K4, uint64_t seed, double *rvec, double *tvec, int *n_inliers, int *rung, int mem)
{
    SVO_CHECK_ARG(ctx && obj_f && img_f && obj_s && img_s && n_f >= 0 && n_s >= 0 && K4 && rvec && tvec);
    SVO_CHECK_ARG(mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE);
    SVO_HIP(hipSetDevice(ctx->device));
    int rc;
    const int cap = n_f > n_s ? n_f : n_s;
    if ((rc = ctx->s_e.ensure(sizeof(PnpRecord) * 2 + 64)) || (rc = ctx->s_f.ensure((size_t)(cap + 1) * 4)) ||
        (rc = ctx->s_g.ensure(64)))
        return rc;
    const float *of = obj_f, *uf = img_f, *os = obj_s, *us = img_s;
    if (mem == SVO_MEM_HOST) {
        if ((rc = ctx->s_a.ensure((size_t)(n_f + 1) * 12)) || (rc = ctx->s_b.ensure((size_t)(n_f + 1) * 8)) ||
            (rc = ctx->s_c.ensure((size_t)(n_s + 1) * 12)) || (rc = ctx->s_d.ensure((size_t)(n_s + 1) * 8)))
            return rc;
        SVO_HIP(hipMemcpyAsync(ctx->s_a.p, obj_f, (size_t)n_f * 12, hipMemcpyHostToDevice, ctx->stream));
        SVO_HIP(hipMemcpyAsync(ctx->s_b.p, img_f, (size_t)n_f * 8, hipMemcpyHostToDevice, ctx->stream));
        SVO_HIP(hipMemcpyAsync(ctx->s_c.p, obj_s, (size_t)n_s * 12, hipMemcpyHostToDevice, ctx->stream));
        SVO_HIP(hipMemcpyAsync(ctx->s_d.p, img_s, (size_t)n_s * 8, hipMemcpyHostToDevice, ctx->stream));
        of = ctx->s_a.as<float>();
        uf = ctx->s_b.as<float>();
        os = ctx->s_c.as<float>();
        us = ctx->s_d.as<float>();
    }
    int *d_cnt = ctx->s_g.as<int>();
    const int hc[2] = {n_f, n_s};
    SVO_HIP(hipMemcpyAsync(d_cnt, hc, sizeof(hc), hipMemcpyHostToDevice, ctx->stream));
    SVO_HIP(hipStreamSynchronize(ctx->stream));  // hc is a stack array
    int r = 0, rin = 0;
    // the launchers skip empty sets: the capacity is at least 1, the live count sits on the device
    if ((rc = ladder_pose(ctx, of, uf, d_cnt, os, us, d_cnt + 1, cap > 0 ? cap : 1, K4, seed + 1, seed + 2,
                          ctx->s_f.as<int>(), reinterpret_cast<PnpRecord *>(ctx->s_e.p), &r, &rin)))
        return rc;
    const PnpRecord *rec = reinterpret_cast<const PnpRecord *>(ctx->pinned);
    if (rung)
        *rung = r;
    if (n_inliers)
        *n_inliers = rin;
    if (rec->n_inliers == 0) {
        svo_set_error("pose ladder: no solution (rung %d, %d points)", r, rec->n_tracked);
        return SVO_ERR_TRACKING_LOST;
    }
    memcpy(rvec, rec->rvec, sizeof(rec->rvec));
    memcpy(tvec, rec->tvec, sizeof(rec->tvec));
    return SVO_OK;
}

void svo_closure_default_params(svo_closure_params *p)
{
    if (!p)
        return;
    p->f_thr = 1.0;          // src/tracking.cpp:75
    p->pnp_iterations = 100; // dump.cpp:340
    p->pnp_reproj_err = 0.1;
    p->pnp_confidence = 0.999;
    p->seed = 0;
}

// getLCMeasurement (dump.cpp:331-348) from the stages svo_vo_localize is made of: PyrLKtrackFrame2Frame (LK, compaction by
// status, F-matrix RANSAC, compaction by mask), solvePnPRansac, Rodrigues / transpose / -R tvec, and the pose as the 7 numbers
// of a pose-graph measurement.  A closure is measured once per detected loop: the call owns its pyramids and work buffer.
int svo_closure_measure(svo_ctx *ctx, const uint8_t *newest, const uint8_t *matched, int w, int h, int c, const float *xy2,
                        const float *xyz3, int n, const double *K4, const svo_closure_params *p, double *meas7, int *n_tracked,
                        int *n_inliers, int mem)
{
    SVO_CHECK_ARG(ctx && newest && matched && w > 0 && h > 0 && (c == 1 || c == 3) && n >= 0 && K4 && meas7);
    SVO_CHECK_ARG(n == 0 || (xy2 && xyz3));
    SVO_CHECK_ARG(mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE);
    svo_closure_params prm;
    svo_closure_default_params(&prm);
    if (p)
        prm = *p;
    SVO_CHECK_ARG(prm.pnp_iterations > 0 && prm.pnp_reproj_err > 0 && prm.pnp_confidence > 0 && prm.pnp_confidence < 1);
    SVO_HIP(hipSetDevice(ctx->device));
    if (n_tracked)
        *n_tracked = 0;
    if (n_inliers)
        *n_inliers = 0;
    if (n == 0) {
        svo_set_error("closure measurement: no points");
        return SVO_ERR_TRACKING_LOST;
    }
    struct Owned {  // released on every way out
        svo_ctx *ctx;
        svo_pyramid *pn = nullptr, *pm = nullptr;
        DevBuf buf;
        ~Owned()
        {
            (void)hipStreamSynchronize(ctx->stream);
            if (pn)
                svo_pyramid_destroy(ctx, pn);
            if (pm)
                svo_pyramid_destroy(ctx, pm);
            buf.release();
        }
    } own{ctx};
    int rc;
    if ((rc = svo_pyramid_create(ctx, w, h, c, SVO_MAX_LEVELS, &own.pn)) ||
        (rc = svo_pyramid_create(ctx, w, h, c, SVO_MAX_LEVELS, &own.pm)))
        return rc;
    // one block: [images] [points in] then the sets of the stages, every piece 256-byte aligned
    const size_t img = ((size_t)w * h * c + 255) & ~(size_t)255, np = (size_t)n + 1;
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t s2 = al(np * 8), s3 = al(np * 12), s1 = al(np), si = al(np * 4);
    const size_t total = 2 * img + 6 * s2 + 3 * s3 + 2 * s1 + si + al(sizeof(PnpRecord)) + 256;
    if ((rc = own.buf.ensure(total)))
        return rc;
    uint8_t *base = own.buf.as<uint8_t>(), *cur = base;
    auto take = [&](size_t b) {
        uint8_t *r = cur;
        cur += b;
        return r;
    };
    uint8_t *d_img0 = take(img), *d_img1 = take(img);
    float *in2 = reinterpret_cast<float *>(take(s2)), *nxt = reinterpret_cast<float *>(take(s2));
    float *a_ref = reinterpret_cast<float *>(take(s2)), *a_trk = reinterpret_cast<float *>(take(s2));
    float *b_ref = reinterpret_cast<float *>(take(s2)), *b_trk = reinterpret_cast<float *>(take(s2));
    float *in3 = reinterpret_cast<float *>(take(s3)), *a_3d = reinterpret_cast<float *>(take(s3));
    float *b_3d = reinterpret_cast<float *>(take(s3));
    uint8_t *status = take(s1), *mask = take(s1);
    int *idx = reinterpret_cast<int *>(take(si));
    PnpRecord *d_rec = reinterpret_cast<PnpRecord *>(take(al(sizeof(PnpRecord))));
    int *d_cnt = reinterpret_cast<int *>(take(256));
    hipStream_t st = ctx->stream;
    SVO_HIP(hipMemsetAsync(d_rec, 0, al(sizeof(PnpRecord)) + 256, st));  // the record and the counts
    const uint8_t *i0 = newest, *i1 = matched;
    const float *p2 = xy2, *p3 = xyz3;
    if (mem == SVO_MEM_HOST) {
        SVO_HIP(hipMemcpyAsync(d_img0, newest, (size_t)w * h * c, hipMemcpyHostToDevice, st));
        SVO_HIP(hipMemcpyAsync(d_img1, matched, (size_t)w * h * c, hipMemcpyHostToDevice, st));
        SVO_HIP(hipMemcpyAsync(in2, xy2, (size_t)n * 8, hipMemcpyHostToDevice, st));
        SVO_HIP(hipMemcpyAsync(in3, xyz3, (size_t)n * 12, hipMemcpyHostToDevice, st));
        i0 = d_img0;
        i1 = d_img1;
        p2 = in2;
        p3 = in3;
    }
    if ((rc = svo_build_pyramid_from_device(ctx, own.pn, i0)) || (rc = svo_build_pyramid_from_device(ctx, own.pm, i1)))
        return rc;
    // PyrLKtrackFrame2Frame (src/tracking.cpp:46-91)
    if ((rc = svo_launch_lk(ctx, own.pn, own.pm, p2, n, nxt, status, nullptr, nullptr)) ||
        (rc = svo_launch_compact(ctx, status, n, nullptr, p2, 2, a_ref, nxt, 2, a_trk, p3, 3, a_3d, d_cnt)))
        return rc;
    const float *trk2 = a_trk, *trk3 = a_3d;
    const int *d_n = d_cnt;
    if (prm.f_thr > 0) {
        if ((rc = svo_launch_fransac(ctx, a_ref, a_trk, n, d_cnt, prm.f_thr, 0.99, 1000, prm.seed + 1, mask, nullptr, nullptr,
                                     nullptr)) ||
            (rc = svo_launch_compact(ctx, mask, n, d_cnt, a_ref, 2, b_ref, a_trk, 2, b_trk, a_3d, 3, b_3d, d_cnt + 1)))
            return rc;
        trk2 = b_trk;
        trk3 = b_3d;
        d_n = d_cnt + 1;
    }
    // solvePnPRansac (dump.cpp:340)
    if ((rc = svo_launch_pnp_ransac(ctx, trk3, trk2, n, d_n, K4, prm.pnp_iterations, prm.pnp_reproj_err, prm.pnp_confidence,
                                    prm.seed + 2, 20, idx, nullptr, d_rec)))
        return rc;
    hipLaunchKernelGGL(store_count_kernel, dim3(1), dim3(1), 0, st, d_n, &d_rec->n_tracked);
    SVO_HIP(hipMemcpyAsync(ctx->pinned, d_rec, sizeof(PnpRecord), hipMemcpyDeviceToHost, st));
    SVO_HIP(hipStreamSynchronize(st));
    const PnpRecord rec = *reinterpret_cast<const PnpRecord *>(ctx->pinned);
    if (n_tracked)
        *n_tracked = rec.n_tracked;
    if (n_inliers)
        *n_inliers = rec.n_inliers;
    if (rec.n_inliers < 6) {
        svo_set_error("closure measurement: %d PnP inliers of %d tracked points", rec.n_inliers, rec.n_tracked);
        return SVO_ERR_TRACKING_LOST;
    }
    // Rodrigues; R = R^T; t = -R * tvec (dump.cpp:342-345)
    double R[9], t[3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
            R[3 * i + j] = rec.R[3 * j + i];
    for (int i = 0; i < 3; i++)
        t[i] = -(R[3 * i] * rec.tvec[0] + R[3 * i + 1] * rec.tvec[1] + R[3 * i + 2] * rec.tvec[2]);
    // the quaternion of R (svo.h states the order of operations)
    double q[4];
    const double tr = R[0] + R[4] + R[8];
    if (tr > 0) {
        const double s = 2. * sqrt(tr + 1.);
        q[0] = (R[7] - R[5]) / s;
        q[1] = (R[2] - R[6]) / s;
        q[2] = (R[3] - R[1]) / s;
        q[3] = s / 4.;
    } else if (R[0] > R[4] && R[0] > R[8]) {
        const double s = 2. * sqrt(1. + R[0] - R[4] - R[8]);
        q[0] = s / 4.;
        q[1] = (R[1] + R[3]) / s;
        q[2] = (R[2] + R[6]) / s;
        q[3] = (R[7] - R[5]) / s;
    } else if (R[4] > R[8]) {
        const double s = 2. * sqrt(1. + R[4] - R[0] - R[8]);
        q[0] = (R[1] + R[3]) / s;
        q[1] = s / 4.;
        q[2] = (R[5] + R[7]) / s;
        q[3] = (R[2] - R[6]) / s;
    } else {
        const double s = 2. * sqrt(1. + R[8] - R[0] - R[4]);
        q[0] = (R[2] + R[6]) / s;
        q[1] = (R[5] + R[7]) / s;
        q[2] = s / 4.;
        q[3] = (R[3] - R[1]) / s;
    }
    const double nrm = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    const double sgn = q[3] / nrm < 0 ? -1. : 1.;
    for (int k = 0; k < 3; k++)
        meas7[k] = t[k];
    for (int k = 0; k < 4; k++)
        meas7[3 + k] = sgn * (q[k] / nrm);
    return SVO_OK;
}

int svo_vo_get_keyframe_cloud(svo_vo *v, float *xyz_cam, int cap, int *n, int mem)
{
    SVO_CHECK_ARG(v && n);
    SVO_CHECK_ARG(mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE);
    *n = v->kf_n;
    if (!xyz_cam)
        return SVO_OK;
    if (cap < v->kf_n) {
        svo_set_error("keyframe cloud has %d points, capacity %d", v->kf_n, cap);
        return SVO_ERR_CAPACITY;
    }
    if (v->kf_n == 0)
        return SVO_OK;
    SVO_HIP(hipMemcpyAsync(xyz_cam, v->b3, (size_t)v->kf_n * 12,
                           mem == SVO_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, v->ctx->stream));
    if (mem == SVO_MEM_HOST)
        SVO_HIP(hipStreamSynchronize(v->ctx->stream));
    return SVO_OK;
}

int svo_vo_get_keyframe_colors(svo_vo *v, float *bgr, int cap, int *n, int mem)
{
    SVO_CHECK_ARG(v && n);
    SVO_CHECK_ARG(mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE);
    *n = v->kf_n;
    if (!bgr)
        return SVO_OK;
    if (cap < v->kf_n) {
        svo_set_error("keyframe colours: %d points, capacity %d", v->kf_n, cap);
        return SVO_ERR_CAPACITY;
    }
    if (v->kf_n == 0)
        return SVO_OK;
    SVO_HIP(hipMemcpyAsync(bgr, v->kf_col, (size_t)v->kf_n * 12,
                           mem == SVO_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, v->ctx->stream));
    if (mem == SVO_MEM_HOST)
        SVO_HIP(hipStreamSynchronize(v->ctx->stream));
    return SVO_OK;
}

int svo_vo_capacity(const svo_vo *v) { return v ? v->cap : 0; }

int svo_vo_set_stage_stamps(svo_vo *v, int enable)
{
    SVO_CHECK_ARG(v);
    v->stamps_on = enable != 0;
    v->stage_frames = 0;
    return SVO_OK;
}

int svo_vo_get_stage_us(const svo_vo *v, double *us, int cap, int *n_frames)
{
    SVO_CHECK_ARG(v && us && cap >= SVO_STAGE_COUNT);
    for (int i = 0; i < SVO_STAGE_COUNT; i++)
        us[i] = v->stage_us[i];
    if (n_frames)
        *n_frames = v->stage_frames;
    return SVO_OK;
}

// ---- the lock-step launches with their gates, as entry points of their own (tests and tools) --------------------------------

int svo_pyramid_build_gated(svo_ctx *ctx, svo_pyramid *pyr, const uint8_t *d_image, const int *d_gate)
{
    SVO_CHECK_ARG(ctx && pyr && d_image);
    return svo_build_pyramids_from_device(ctx, 1, &pyr, &d_image, &d_gate);
}

int svo_lk_track_jobs(svo_ctx *ctx, int n_jobs, svo_pyramid *const *prev, const svo_pyramid *const *next,
                      const float *const *d_prev_pts, const int *n, float *const *d_next_pts, uint8_t *const *d_status,
                      float *const *d_err, float *const *d_min_eig, const int *const *d_gates)
{
    SVO_CHECK_ARG(ctx && n_jobs >= 1 && n_jobs <= SVO_LK_MAX_JOBS && prev && next && d_prev_pts && n && d_next_pts && d_status);
    LkJob lk[SVO_LK_MAX_JOBS];
    for (int a = 0; a < n_jobs; a++) {
        SVO_CHECK_ARG(prev[a] && next[a] && d_prev_pts[a] && d_next_pts[a] && d_status[a] && n[a] >= 0);
        SVO_CHECK_ARG(prev[a]->w == next[a]->w && prev[a]->h == next[a]->h && prev[a]->c == next[a]->c &&
                      prev[a]->levels == next[a]->levels);
        if (!prev[a]->has_deriv) {
            svo_pyramid *pv = prev[a];
            int rc = svo_build_derivatives(ctx, 1, &pv);
            if (rc)
                return rc;
        }
        LkJob &q = lk[a];
        q.prev = prev[a]->dev;
        q.next = next[a]->dev;
        q.dprev = prev[a]->dbase;
        q.prev_pts = d_prev_pts[a];
        q.n_cap = n[a];
        q.d_n = nullptr;
        q.next_pts = d_next_pts[a];
        q.status = d_status[a];
        q.err = d_err ? d_err[a] : nullptr;
        q.min_eig = d_min_eig ? d_min_eig[a] : nullptr;
        q.gate = d_gates ? d_gates[a] : nullptr;
    }
    return svo_launch_lk_batch(ctx, n_jobs, lk, prev[0]);
}

}  // extern "C"
