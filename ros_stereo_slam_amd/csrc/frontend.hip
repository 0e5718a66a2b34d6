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
//
// The state and the helpers shared with the chain runner (frontend_chain.hip): frontend_state.hip.h.  Here: the stereo
// path, the frame-by-frame entry points, and the entry points that borrow the pose ladder.
#include <cmath>

#include "frontend_state.hip.h"

namespace {

int grid_axis(int dim, int step)
{
    int k = 0;
    for (int v = step; v < dim - step; v += step)
        k++;
    return k;
}

__global__ void store_count_kernel(const int *__restrict__ src, int *__restrict__ dst) { *dst = *src; }

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

// The 2-D part of visualSLAM::stereoTriangulate, dense branch (src/triangulation.cpp:87-103,137-141), for up to NJ
// front-ends at once: the argument arrays of its launches, one slot per front-end.
template <int NJ> struct StereoJobs {
    LkJob lk[NJ];
    const float *xy[NJ], *resp[NJ];  // ANMS (only with an ANMS budget)
    int *oidx[NJ], *ocnt[NJ];
    svo_anms_gather ga[NJ];
    const int *gates[NJ];
    svo_compact_job c1[NJ], c2[NJ];
    svo_fransac_job fj[NJ];
    float *x1[NJ], *x2[NJ];  // where the filtered pairs and their count land: what the triangulation reads
    int *cnt[NJ];
};

// Slot a of the jobs: the stereo path of front-end v from the pyramids left / right in the buffers B.  Every kernel runs only
// while *gate is set (null: always); x1 / x2 / cnt: the destinations of the filtered pairs and their count (x2 null: the
// free half of the ping-pong pairs).
template <int NJ>
void stereo_jobs(StereoJobs<NJ> &J, int a, const svo_vo *v, const StereoBufs &B, const svo_pyramid *left,
                 const svo_pyramid *right, const int *gate, uint64_t seed, float *x1, float *x2, int *cnt)
{
    const int n = vo_grid_points(v);
    // denseLKtracking: LK left -> right (src/tracking.cpp:18); min-eig is the ANMS response
    J.lk[a] = lk_job(left, right, v->grid_xy, n, nullptr, B.b2, B.status, B.resp, gate);
    J.gates[a] = gate;
    const float *pts = v->grid_xy, *trk = B.b2;
    const uint8_t *stt = B.status;
    const int *d_n = nullptr;
    if (v->prm.anms_keep > 0) {
        // the kept keypoints' lattice points, tracked points and status bytes come out of the same launch
        // that lists them (a gather launch of its own before)
        J.xy[a] = v->grid_xy;
        J.resp[a] = B.resp;
        J.oidx[a] = B.idx;
        J.ocnt[a] = B.cnt + CNT_ANMS;
        J.ga[a] = {v->grid_xy, B.b2, B.c2, B.d2, B.status, B.st2};
        pts = B.c2;
        trk = B.d2;
        stt = B.st2;
        d_n = B.cnt + CNT_ANMS;
    }
    // status compaction (src/tracking.cpp:20-27); ping-pong between the (a2,b2) and (c2,d2) pairs
    float *o1 = pts == v->grid_xy ? B.c2 : B.a2, *o2 = pts == v->grid_xy ? B.d2 : B.b2;
    if (!x2)
        x2 = o1 == B.a2 ? B.c2 : B.a2;
    J.c1[a] = {stt, n, d_n, {pts, trk, nullptr}, {o1, o2, nullptr}, {2, 2, 0}, B.cnt + CNT_ST_STATUS, gate};
    // FmatThresholding (src/tracking.cpp:30-43): 3 px, 0.99
    J.c2[a] = {B.mask, n, B.cnt + CNT_ST_STATUS, {o1, o2, nullptr}, {x1, x2, nullptr}, {2, 2, 0}, cnt};
    J.fj[a] = {o1, o2, n, B.cnt + CNT_ST_STATUS, v->prm.f_thr_stereo, 0.99, 1000, seed, B.mask, nullptr, nullptr,
               nullptr, &J.c2[a], gate};  // the mask compaction rides with the F-RANSAC
    J.x1[a] = x1;
    J.x2[a] = x2;
    J.cnt[a] = cnt;
}

// the launches of k slots, on the context's current stream: every stage is one set of launches
template <int NJ> int stereo_launch(svo_ctx *ctx, int k, const StereoJobs<NJ> &J, const svo_vo *v0, const svo_pyramid *geom)
{
    int rc;
    if ((rc = svo_launch_lk_batch(ctx, k, J.lk, geom)))
        return rc;
    if (v0->prm.anms_keep > 0 && (rc = svo_launch_anms_batch(ctx, k, J.xy, J.resp, vo_grid_points(v0), v0->prm.anms_keep,
                                                             J.oidx, J.ocnt, J.ga, J.gates)))
        return rc;
    if ((rc = svo_launch_compact_batch(ctx, k, J.c1)) || (rc = svo_launch_fransac_batch(ctx, k, J.fj)))
        return rc;
    return SVO_OK;
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
    const float *o3 = obj_f, *o2 = img_f;
    const int *cnt = cnt_f;
    *rung = 0;
    if ((rc = svo_launch_pnp_ransac(ctx, o3, o2, cap, cnt, K4, 100, 4.0, 0.99, seed1, 20, idx_scratch, nullptr, d_rec)) ||
        (rc = vo_fetch_record(ctx, d_rec, cnt)))
        return rc;
    bool plain = false;
    if (rec->n_inliers < 20 || rec->tvec[0] > 1000) {
        *rung = 1;
        o3 = obj_s;
        o2 = img_s;
        cnt = cnt_s;
        if ((rc = svo_launch_pnp_ransac(ctx, o3, o2, cap, cnt, K4, 100, 4.0, 0.99, seed2, 20, idx_scratch, nullptr,
                                        d_rec)) ||
            (rc = vo_fetch_record(ctx, d_rec, cnt)))
            return rc;
        plain = rec->n_inliers < 10 || rec->tvec[0] > 1000;
    }
    const int ninl = rec->n_inliers;
    if (ransac_inliers)
        *ransac_inliers = ninl;
    if (plain || ninl < 10) {  // "Skipping RANSAC all together": cv::solvePnP on everything that was tracked
        *rung = 2;
        if ((rc = svo_launch_solve_pnp(ctx, o3, o2, cap, cnt, K4, 20, idx_scratch, d_rec)) ||
            (rc = vo_fetch_record(ctx, d_rec, cnt)))
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

int vo_grid_points(const svo_vo *v) { return grid_axis(v->w, v->prm.grid_step) * grid_axis(v->h, v->prm.grid_step); }

int vo_fetch_record(svo_ctx *ctx, PnpRecord *d_rec, const int *d_cnt)
{
    hipLaunchKernelGGL(store_count_kernel, dim3(1), dim3(1), 0, ctx->stream, d_cnt, &d_rec->n_tracked);
    SVO_HIP(hipMemcpyAsync(ctx->pinned, d_rec, sizeof(PnpRecord), hipMemcpyDeviceToHost, ctx->stream));
    return svo_wait(ctx);
}

int vo_check_reference(int nref)
{
    if (nref >= 5)
        return SVO_OK;
    svo_set_error("tracking lost: %d reference points", nref);
    return SVO_ERR_TRACKING_LOST;
}

// identity [R|t]: the world cloud equals the camera-frame one bit for bit (x * 1 + y * 0 + z * 0 + 0 in
// double), and the camera-frame cloud lands in b3 as at every later keyframe (svo_vo_get_keyframe_cloud)
const double kIdentityRt[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};

void vo_reset_pose(svo_vo *v)
{
    for (int i = 0; i < 9; i++)
        v->R[i] = (i % 4) == 0;
    v->t[0] = v->t[1] = v->t[2] = 0;
}

// visualSLAM::stereoTriangulate, dense branch (src/triangulation.cpp:87-103,137-165), with
// the optional ANMS stage, for k front-ends of one context at once (same image size, grid step
// and ANMS budget): every stage is one set of launches.  Per front-end: x1 -> out2d, camera-frame
// points -> v->b3 and, when Rt is given, world points -> out3d (else the camera-frame points).
// Count -> d_cnt[CNT_ST_MASK] and host.
// chained: the chain runner's form -- every kernel of job a runs only when vs[a]->d_chain->kf is set, [R|t] is the
// pose the device holds (Rts ignored), the count goes to the chain state, nothing is waited for (n_out untouched).
int stereo_triangulate_batch(int k, svo_vo *const *vs, svo_pyramid *const *lefts, svo_pyramid *const *rights,
                             const double *const *Rts, float *const *out2d, float *const *out3d, int *const *n_out,
                             bool chained)
{
    svo_vo *v0 = vs[0];
    svo_ctx *ctx = v0->ctx;
    int rc;
    const int n = vo_grid_points(v0);
    StereoJobs<SVO_LK_MAX_JOBS> J;
    svo_tri_job tj[SVO_LK_MAX_JOBS];
    for (int a = 0; a < k; a++) {
        svo_vo *v = vs[a];
        stereo_jobs(J, a, v, own_stereo_bufs(v), lefts[a], rights[a], chained ? &v->d_chain->kf : nullptr,
                    stage_seed(v, v->frame, 3), out2d[a], nullptr, v->d_cnt + CNT_ST_MASK);
        if (chained)  // [R|t] and the gate come from the chain state; the count goes there
            tj[a] = {J.x1[a], J.x2[a], n, J.cnt[a], v->b3, nullptr, nullptr, out3d[a], nullptr, v->d_chain};
        else
            tj[a] = {J.x1[a], J.x2[a], n, J.cnt[a], Rts[a] ? v->b3 : out3d[a], nullptr, Rts[a], Rts[a] ? out3d[a] : nullptr,
                     reinterpret_cast<int *>(ctx->pinned) + a};  // the count the host reads after the wait below
        tj[a].color_src = lefts[a];  // `colors` of stereoTriangulate (src/triangulation.cpp:139-140), same launch
        tj[a].color_out = v->kf_col;
    }
    double P1[12], P2[12];
    svo_stereo_projections(v0->prm.fx, v0->prm.fy, v0->prm.cx, v0->prm.cy, v0->prm.baseline, P1, P2);
    if ((rc = stereo_launch(ctx, k, J, v0, lefts[0])) || (rc = svo_launch_triangulate_batch(ctx, P1, P2, k, tj)))
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

// The stereo path of a keyframe candidate for ONE pipelined chunk, on the lane's stream and buffers: LK left -> right from
// the lattice (src/tracking.cpp:18), ANMS, status filter (:20-27), F-RANSAC at 3 px with its mask filter (:30-43), the
// DLT triangulation in the camera frame (src/triangulation.cpp:142-160) -- all of stereoTriangulate, none of which
// needs the frame's pose.  Leaves x1 / x2 / count in h_x1 / h_x2 / h_cnt[slot]; every kernel runs while the chain is live.
// `frame_no`: the frame the pass belongs to (its seed).
int stereo_part1_spec(svo_vo *v, svo_pyramid *left, svo_pyramid *right, int frame_no, int slot)
{
    StereoJobs<1> J;
    stereo_jobs(J, 0, v, v->lane.buf, left, right, &v->d_chain->run, stage_seed(v, frame_no, 3), v->h_x1[slot], v->h_x2[slot],
                v->h_cnt + slot);
    return stereo_launch(v->lane.ctx, 1, J, v, left);
}

// ... its last stage, the DLT triangulation of the filtered pairs in the camera frame (src/triangulation.cpp:142-160), on
// the context's current stream (the pipelined chunk runs it on the pyramid stream: the stereo stream is the busiest)
int stereo_tri_spec(svo_vo *v, int slot)
{
    const svo_tri_job tj = {v->h_x1[slot], v->h_x2[slot], vo_grid_points(v), v->h_cnt + slot, v->h_xyz[slot], nullptr, nullptr,
                            nullptr, nullptr};
    double P1[12], P2[12];
    svo_stereo_projections(v->prm.fx, v->prm.fy, v->prm.cx, v->prm.cy, v->prm.baseline, P1, P2);
    return svo_launch_triangulate_batch(v->ctx, P1, P2, 1, &tj);
}

// ... and what is left once the frame is decided, only when the device flag says keyframe: what = 1, the hand-over of
// the 2-D set (all the next tracking pass needs); what = 2, the cloud placed with the frame's refined pose
// (src/keyFrameManagement.cpp:18-30).  On the context's current stream.
int stereo_part2_spec(svo_vo *v, const svo_pyramid *left, int slot, int what)
{
    return svo_launch_keyframe_place(v->ctx, v->d_chain, v->h_x1[slot], v->h_xyz[slot], vo_grid_points(v), v->h_cnt + slot,
                                     v->ref2d, v->b3, v->ref3d, left, v->kf_col, what);
}

int vo_pipe_prepare(svo_vo *v)
{
    if (v->pipe_ready)
        return SVO_OK;
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
    StereoBufs &B = L.buf;
    if (!L.ctx && (rc = svo_ctx_create(v->ctx->device, &L.ctx)))
        return rc;
    if ((!B.a2 && (rc = dev_alloc(&B.a2, n * 2))) || (!B.b2 && (rc = dev_alloc(&B.b2, n * 2))) ||
        (!B.c2 && (rc = dev_alloc(&B.c2, n * 2))) || (!B.d2 && (rc = dev_alloc(&B.d2, n * 2))) ||
        (!B.resp && (rc = dev_alloc(&B.resp, n))) || (!B.status && (rc = dev_alloc(&B.status, n))) ||
        (!B.st2 && (rc = dev_alloc(&B.st2, n))) || (!B.mask && (rc = dev_alloc(&B.mask, n))) ||
        (!B.idx && (rc = dev_alloc(&B.idx, n))) || (!B.cnt && (rc = dev_alloc(&B.cnt, kCntSlots))))
        return rc;
    for (int k = 0; k < 3; k++)
        if ((!v->h_x2[k] && (rc = dev_alloc(&v->h_x2[k], n * 2))) || (!v->h_x1[k] && (rc = dev_alloc(&v->h_x1[k], n * 2))) ||
            (!v->h_xyz[k] && (rc = dev_alloc(&v->h_xyz[k], n * 3))))
            return rc;
    if ((!v->h_cnt && (rc = dev_alloc(&v->h_cnt, 16))) || (!v->trk2d_b && (rc = dev_alloc(&v->trk2d_b, n * 2))) ||
        (!v->trk3d_b && (rc = dev_alloc(&v->trk3d_b, n * 3))) || (!v->idx_b && (rc = dev_alloc(&v->idx_b, n))) ||
        (!v->status_b && (rc = dev_alloc(&v->status_b, n))))
        return rc;
    for (int k = 0; k < 3; k++)
        if ((!v->a2k[k] && (rc = dev_alloc(&v->a2k[k], n * 2))) || (!v->statusk[k] && (rc = dev_alloc(&v->statusk[k], n))))
            return rc;
    for (hipEvent_t &e : v->ev)
        if (!e)
            SVO_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    v->pipe_ready = true;
    return SVO_OK;
}

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
        (rc = dev_alloc(&v->st2, n)) || (rc = dev_alloc(&v->idx, n)) || (rc = dev_alloc(&v->d_cnt, kCntSlots)) ||
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
    vo_reset_pose(v);
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
    for (hipStream_t st : {v->stream_b, v->stream_p})
        if (st) {
            (void)hipStreamSynchronize(st);
            (void)hipStreamDestroy(st);
        }
    for (hipEvent_t e : v->ev)
        if (e)
            (void)hipEventDestroy(e);
    {
        svo_vo::StereoLane &L = v->lane;
        if (L.ctx) {
            (void)hipStreamSynchronize(L.ctx->stream);
            (void)svo_ctx_destroy(L.ctx);
        }
        const StereoBufs &B = L.buf;
        void *sb[] = {B.a2,        B.b2,        B.c2,        B.d2,         B.resp,       B.status, B.st2,      B.mask,
                      B.idx,       B.cnt,       v->h_x1[0],  v->h_x1[1],   v->h_xyz[0],  v->h_xyz[1], v->h_cnt, v->trk2d_b, v->trk3d_b,
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
    vo_reset_pose(v);
    const uint8_t *d = stage_image(v, left, mem, &rc);
    if (rc || (rc = svo_build_pyramid_from_device(v->ctx, v->pyr_ref, d)))
        return rc;
    d = stage_image(v, right, mem, &rc);
    if (rc || (rc = svo_build_pyramid_from_device(v->ctx, v->pyr_right, d)))
        return rc;
    if ((rc = stereo_triangulate(v, v->pyr_ref, v->pyr_right, kIdentityRt, v->ref2d, v->ref3d, &v->nref)))
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
    if ((rc = vo_check_reference(n)))
        return rc;
    // PyrLKtrackFrame2Frame (src/tracking.cpp:46-91)
    if ((rc = svo_launch_lk(ctx, v->pyr_ref, v->pyr_cur, v->ref2d, n, v->a2, v->status, nullptr, nullptr)))
        return rc;
    if ((rc = svo_launch_compact(ctx, v->status, n, nullptr, v->ref2d, 2, v->b2, v->a2, 2, v->c2, v->ref3d, 3, v->a3,
                                 v->d_cnt + CNT_STATUS)))
        return rc;
    {
        // the F-RANSAC's finishing wave also compacts by its mask (src/tracking.cpp:77-88)
        const svo_compact_job by_mask = {v->mask, n, v->d_cnt + CNT_STATUS, {v->c2, v->a3, nullptr}, {v->trk2d, v->trk3d, nullptr},
                                         {2, 3, 0}, v->d_cnt + CNT_TRK_A};
        if ((rc = svo_launch_fransac(ctx, v->b2, v->c2, n, v->d_cnt + CNT_STATUS, v->prm.f_thr_temporal, 0.99, 1000, stage_seed(v, v->frame, 0),
                                     v->mask, nullptr, nullptr, nullptr, &by_mask)))
            return rc;
    }
    const double K4[4] = {v->prm.fx, v->prm.fy, v->prm.cx, v->prm.cy};
    const PnpRecord *rec = reinterpret_cast<const PnpRecord *>(ctx->pinned);
    if (v->prm.policy == SVO_POLICY_VO_LADDER) {
        // visualOdometry::initSequence, src/bundleAdjust.cpp:452-480 (see svo_vo_params.policy)
        int rung = 0;
        if ((rc = ladder_pose(ctx, v->trk3d, v->trk2d, v->d_cnt + CNT_TRK_A, v->a3, v->c2, v->d_cnt + CNT_STATUS, n, K4,
                              stage_seed(v, v->frame, 1), stage_seed(v, v->frame, 2), v->idx, v->d_rec, &rung,
                              &v->ladder_ransac_inliers)))
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
        pose_from_record(*rec, R9, t3);
        return SVO_OK;
    }
    // solvePnPRansac (src/keyFrameManagement.cpp:84), retry (:85-92)
    for (int attempt = 0; attempt < 2; attempt++) {
        if ((rc = svo_launch_pnp_ransac(ctx, v->trk3d, v->trk2d, n, v->d_cnt + CNT_TRK_A, K4, 100, attempt ? 8.0 : 1.0,
                                        attempt ? 0.98 : 0.99, stage_seed(v, v->frame, attempt ? 2 : 1), 20, v->idx, nullptr,
                                        v->d_rec)) ||
            (rc = vo_fetch_record(ctx, v->d_rec, v->d_cnt + CNT_TRK_A)))
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
    pose_from_record(*rec, R9, t3);
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
    int *cnt = ctx->s_g.as<int>();  // [0] the filtered set's count, [1] the status-filtered set's
    const int hc[2] = {n_f, n_s};
    SVO_HIP(hipMemcpyAsync(cnt, hc, sizeof(hc), hipMemcpyHostToDevice, ctx->stream));
    SVO_HIP(hipStreamSynchronize(ctx->stream));  // hc is a stack array
    int r = 0, rin = 0;
    // the launchers skip empty sets: the capacity is at least 1, the live count sits on the device
    if ((rc = ladder_pose(ctx, of, uf, &cnt[0], os, us, &cnt[1], cap > 0 ? cap : 1, K4, seed + 1, seed + 2,
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
    int *cnt = reinterpret_cast<int *>(take(256));  // [0] after the status filter, [1] after the mask filter
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
        (rc = svo_launch_compact(ctx, status, n, nullptr, p2, 2, a_ref, nxt, 2, a_trk, p3, 3, a_3d, &cnt[0])))
        return rc;
    const float *trk2 = a_trk, *trk3 = a_3d;
    const int *d_n = &cnt[0];
    if (prm.f_thr > 0) {
        if ((rc = svo_launch_fransac(ctx, a_ref, a_trk, n, &cnt[0], prm.f_thr, 0.99, 1000, prm.seed + 1, mask, nullptr, nullptr,
                                     nullptr)) ||
            (rc = svo_launch_compact(ctx, mask, n, &cnt[0], a_ref, 2, b_ref, a_trk, 2, b_trk, a_3d, 3, b_3d, &cnt[1])))
            return rc;
        trk2 = b_trk;
        trk3 = b_3d;
        d_n = &cnt[1];
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
    pose_from_record(rec, R, t);
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
        lk[a] = lk_job(prev[a], next[a], d_prev_pts[a], n[a], nullptr, d_next_pts[a], d_status[a],
                       d_min_eig ? d_min_eig[a] : nullptr, d_gates ? d_gates[a] : nullptr);
        lk[a].err = d_err ? d_err[a] : nullptr;
    }
    return svo_launch_lk_batch(ctx, n_jobs, lk, prev[0]);
}

}  // extern "C"
