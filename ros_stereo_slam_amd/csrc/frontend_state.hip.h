// frontend_state.hip.h -- the stereo-VO front-end's state (svo_vo) and the host helpers its translation units share:
// frontend.hip (the frame-by-frame entry points, the stereo path), frontend_chain.hip (the chain runner).
#pragma once

#include "svo_internal.h"

struct PnpRecord {  // layout of pnp.hip's PnpResult + the tracked-point count behind it
    double rvec[3], tvec[3], R[9], rms;
    int n_inliers, iters_run;
    int n_tracked, pad;
};

// The stage counts of a front-end (svo_vo::d_cnt) and of its stereo lane (StereoBufs::cnt), device ints.
enum CntSlot {
    CNT_STATUS = 0,      // after the temporal status filter
    CNT_TRK_A = 1,       // tracked set A
    CNT_ANMS = 2,        // ANMS kept
    CNT_ST_STATUS = 3,   // after the stereo status filter
    CNT_ST_MASK = 4,     // after the stereo mask filter
    CNT_TRK_B = 9,       // tracked set B (pipelined chunk)
    CNT_3D_STATUS = 10,  // the 3-D column on the PnP stream: after its status filter ...
    CNT_3D_MASK = 11,    // ... and after its mask filter
};
constexpr int kCntSlots = 16;

// the buffers one stereo path works in: the front-end's own, or those of its lane (pipelined chunk)
struct StereoBufs {
    float *a2 = nullptr, *b2 = nullptr, *c2 = nullptr, *d2 = nullptr, *resp = nullptr;
    uint8_t *status = nullptr, *st2 = nullptr, *mask = nullptr;
    int *idx = nullptr, *cnt = nullptr;
};

// the events of a pipelined chunk: tracked sets ready (A), tracking launch ended (A), cloud placed (B), refined (B: end of
// a run); then by frame & 3: pyramids built (D), triangulated (D), keyframe handed over (B), keyframe pass done (E), stereo
// path done (C)
enum PipeEvent { EV_FLT, EV_LK, EV_DEC, EV_REF, EV_PYR = 4, EV_P1 = 8, EV_P3 = 12, EV_E = 16, EV_C = 20, EV_COUNT = 24 };

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
        StereoBufs buf;
    } lane;
    // what the lane hands to A and B, by frame % 3: the keyframe candidate's 2-D points, camera-frame points, count
    float *h_x1[3] = {nullptr, nullptr, nullptr}, *h_xyz[3] = {nullptr, nullptr, nullptr}, *h_x2[3] = {nullptr, nullptr, nullptr};
    int *h_cnt = nullptr;
    // output of the tracking pass from the keyframe candidate's points (beside a2 / status of the pass from the tracked set)
    float *a2k[3] = {nullptr, nullptr, nullptr};  // by target frame % 3 (stream E writes a frame's two frames ahead)
    // status bytes of both passes by frame parity: the PnP stream reads a frame's while A's next launch writes the next frame's
    uint8_t *statusk[3] = {nullptr, nullptr, nullptr}, *status_b = nullptr;
    hipEvent_t ev[EV_COUNT] = {nullptr};  // PipeEvent
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
    int *idx = nullptr, *d_cnt = nullptr;  // d_cnt[kCntSlots]: stage counts, by CntSlot
    PnpRecord *d_rec = nullptr;  // one per tracked set
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

// one of the two tracked sets of a front-end (pipelined chunks alternate; everything else uses set 0): 2-D and 3-D points,
// the PnP's inlier list, the set's count and the PnP's record
struct TrackedSet {
    float *p2, *p3;
    int *idx, *cnt;
    PnpRecord *rec;
};
inline TrackedSet tracked_set(const svo_vo *v, int set)
{
    if (set)
        return {v->trk2d_b, v->trk3d_b, v->idx_b, v->d_cnt + CNT_TRK_B, v->d_rec + 1};
    return {v->trk2d, v->trk3d, v->idx, v->d_cnt + CNT_TRK_A, v->d_rec};
}

inline StereoBufs own_stereo_bufs(const svo_vo *v)
{
    return {v->a2, v->b2, v->c2, v->d2, v->resp, v->status, v->st2, v->mask, v->idx, v->d_cnt};
}

template <class T> int dev_alloc(T **p, size_t count)
{
    hipError_t e = hipMalloc((void **)p, count * sizeof(T));
    if (e != hipSuccess) {
        svo_set_error("hipMalloc(%zu) -> %s", count * sizeof(T), hipGetErrorString(e));
        return SVO_ERR_HIP;
    }
    return SVO_OK;
}

inline uint64_t stage_seed(const svo_vo *v, int frame, int stage) { return v->prm.seed + 8ull * (uint64_t)frame + stage; }

// one pyramidal-LK pass prev -> next from `pts` (n_cap points, or *d_n when given)
inline LkJob lk_job(const svo_pyramid *prev, const svo_pyramid *next, const float *pts, int n_cap, const int *d_n,
                    float *next_pts, uint8_t *status, float *min_eig, const int *gate)
{
    LkJob q;
    q.prev = prev->dev;
    q.next = next->dev;
    q.dprev = prev->dbase;
    q.prev_pts = pts;
    q.n_cap = n_cap;
    q.d_n = d_n;
    q.next_pts = next_pts;
    q.status = status;
    q.err = nullptr;
    q.min_eig = min_eig;
    q.gate = gate;
    return q;
}

// Rodrigues; R = R^T; t = -R * tvec (src/VisualSLAM.cpp:70-74)
inline void pose_from_record(const PnpRecord &rec, double *R9, double *t3)
{
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
            R9[3 * i + j] = rec.R[3 * j + i];
    for (int i = 0; i < 3; i++)
        t3[i] = -(R9[3 * i] * rec.tvec[0] + R9[3 * i + 1] * rec.tvec[1] + R9[3 * i + 2] * rec.tvec[2]);
}

// ---- frontend.hip ----
// points of the keypoint lattice (src/triangulation.cpp:89-96): the capacity of every stereo-path launch
int vo_grid_points(const svo_vo *v);
// the count behind the record, the record into the context's pinned block, and the wait for it
int vo_fetch_record(svo_ctx *ctx, PnpRecord *d_rec, const int *d_cnt);
// fewer than 5 reference points: the error text and SVO_ERR_TRACKING_LOST, else SVO_OK
int vo_check_reference(int nref);
// the identity pose; kIdentityRt: that pose as the [R|t] of a keyframe
void vo_reset_pose(svo_vo *v);
extern const double kIdentityRt[12];
// the streams, buffers and events of a pipelined chunk, made when pipelining is first asked for (svo_vo_destroy releases them)
int vo_pipe_prepare(svo_vo *v);
// visualSLAM::stereoTriangulate for k front-ends of one context at once; chained: the chain runner's form
int stereo_triangulate_batch(int k, svo_vo *const *vs, svo_pyramid *const *lefts, svo_pyramid *const *rights,
                             const double *const *Rts, float *const *out2d, float *const *out3d, int *const *n_out,
                             bool chained = false);
// the stereo path of a pipelined chunk, in three parts
int stereo_part1_spec(svo_vo *v, svo_pyramid *left, svo_pyramid *right, int frame_no, int slot);
int stereo_tri_spec(svo_vo *v, int slot);
int stereo_part2_spec(svo_vo *v, const svo_pyramid *left, int slot, int what);
