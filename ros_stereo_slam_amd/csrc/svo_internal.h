// svo_internal.h -- shared host-side declarations of libsvo_hip.so (not installed).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/svo.h"
#include "../../include/svo_math.h"  // the transcendental functions of the geometry solvers, shared with the oracle

#define SVO_MAX_LEVELS 4
#define SVO_LK_WIN 21
// Every pyramid level is stored with a reflect-101 border of SVO_PYR_PAD pixels on each
// side and a 16-byte-aligned row pitch, so the LK kernel stages tiles with aligned 16-byte
// loads and no border arithmetic (the furthest it reaches outside the image is 26 px).
#define SVO_PYR_PAD 32
// independent jobs one batched launch may carry (chunks of a context that run in lock step)
#define SVO_LK_MAX_JOBS 16

#define SVO_N_TICKETS 64
static_assert(32 + 2 * SVO_LK_MAX_JOBS <= SVO_N_TICKETS, "svo_ctx::d_tickets: lk_expand_kernel's slots end past the allocation");

void svo_set_error(const char *fmt, ...);

// The short kernels between two tracking launches (F-RANSAC, PnP, ANMS, compaction, pyramids) run beside the
// tracking launches of the other contexts, whose waves keep every SIMD's issue port busy: a latency-bound
// wave that takes its turn among four tracking waves runs at a fifth of its speed.  They raise their issue
// priority instead (s_setprio: the arbiter picks the highest-priority ready wave); the tracker stays at 0.
__device__ __forceinline__ void svo_chain_priority() { __builtin_amdgcn_s_setprio(3); }

// cvtColor(BGR2GRAY) of one 8-bit pixel: OpenCV's fixed-point weights, one rounding
__host__ __device__ __forceinline__ int svo_bgr2gray(int b, int g, int r) { return (1868 * b + 9617 * g + 4899 * r + 8192) >> 14; }

#define SVO_HIP(call)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess) {                                                               \
            svo_set_error("%s:%d %s -> %s", __FILE__, __LINE__, #call, hipGetErrorString(e_)); \
            return SVO_ERR_HIP;                                                               \
        }                                                                                     \
    } while (0)

#define SVO_CHECK_ARG(cond)                                                  \
    do {                                                                     \
        if (!(cond)) {                                                       \
            svo_set_error("%s:%d bad argument: %s", __FILE__, __LINE__, #cond); \
            return SVO_ERR_ARG;                                              \
        }                                                                    \
    } while (0)

// device-visible description of one pyramid (passed to kernels by value)
struct PyrDev {
    const uint8_t *lvl[SVO_MAX_LEVELS];  // address of pixel (0,0); rows/cols -PAD..size+PAD-1 are valid
    int pitch[SVO_MAX_LEVELS];           // bytes per row, multiple of 16
    int w[SVO_MAX_LEVELS];
    int h[SVO_MAX_LEVELS];
    int levels;
    int c;
};

// a 3 x 4 double matrix ([R|t], a projection) passed to kernels by value: geometry.hip, replenish.hip
struct Mat34 {
    double m[12];
};

// A few device words per pyramid live in a header of SVO_PYR_HEADER bytes in front of level 0's padded buffer, i.e. at
// lvl[0] - PAD * pitch[0] - PAD * c - SVO_PYR_HEADER: whoever holds the PyrDev finds them, no pointer of their own.
//   SVO_PYR_MONO         1: the image the pyramid was last built from has B == G == R in every pixel (c == 3 only;
//                        pyramids of 1 or 4 channels, and pyramids never built, say 0).  Published by the finishing launch
//                        of a build, left alone by a gated build and by svo_build_derivatives.
//   SVO_PYR_COLOUR_SEEN  collects during the head launch of a build, cleared when SVO_PYR_MONO is published
//   SVO_PYR_STORED       channels the last build stored: 1 = the grey regions (below) hold the levels and derivative levels,
//                        anything else = the three-channel regions do.  Written by the base launch of a c == 3 build.
//   SVO_PYR_COLOUR_VALID of a grey-stored pyramid: bit 0 = the three-channel levels, bit 1 = the three-channel derivative
//                        levels have been expanded from the grey ones since the last build (lk.hip: lk_expand_kernel)
// Grey storage (c == 3 only): a grey frame given as BGR is stored ONCE, in regions of their own behind the three-channel
// levels (svo_pyramid::goff) and behind the three-channel derivative levels (svo_pyramid::gdoff), each in exactly the
// layout of a one-channel pyramid of the same size: pitches svo_grey_pitch / svo_grey_dpitch.  Pixel (0, 0) of grey level l
// lies svo_pyramid::gdelta[l] bytes behind pixel (0, 0) of level l: the same for every pyramid of one geometry, so the
// kernels get it by value.
#define SVO_PYR_HEADER 256
enum { SVO_PYR_MONO = 0, SVO_PYR_COLOUR_SEEN = 1, SVO_PYR_STORED = 2, SVO_PYR_COLOUR_VALID = 3 };
// `padded`: the first byte of level 0's padded buffer
__host__ __device__ __forceinline__ int *svo_pyr_words(const uint8_t *padded)
{
    return reinterpret_cast<int *>(const_cast<uint8_t *>(padded) - SVO_PYR_HEADER);
}
__host__ __device__ __forceinline__ int svo_grey_pitch(int w) { return (w + 2 * SVO_PYR_PAD + 15) & ~15; }
__host__ __device__ __forceinline__ int svo_grey_dpitch(int w) { return ((w + 2 * 32 /* SVO_DERIV_PAD */) * 4 + 15) & ~15; }
// Level-0 pixel (x, y) of a pyramid of c channels for the colour gathers (geometry.hip): the address of its first byte and
// the step to its next channel (0 where one stored byte stands for all three); gdelta0: svo_pyramid::gdelta[0]
__device__ __forceinline__ const uint8_t *svo_pyr_pixel0(const uint8_t *lvl0, int pitch, int c, int w, int gdelta0, int x, int y,
                                                         int *step)
{
    *step = c >= 3 ? 1 : 0;
    if (c == 3) {
        const int *words = svo_pyr_words(lvl0 - (ptrdiff_t)SVO_PYR_PAD * pitch - SVO_PYR_PAD * c);
        if (words[SVO_PYR_STORED] == 1) {
            *step = 0;
            return lvl0 + gdelta0 + (ptrdiff_t)y * svo_grey_pitch(w) + x;
        }
    }
    return lvl0 + (size_t)y * pitch + x * c;
}

struct svo_pyramid {
    int w, h, c, levels;
    uint8_t *base;   // one HBM allocation, padded levels back to back (256-B aligned each)
    size_t off[SVO_MAX_LEVELS];  // offset of each level's padded buffer
    uint8_t *origin(int l) const
    {
        return base + off[l] + (size_t)SVO_PYR_PAD * dev.pitch[l] + (size_t)SVO_PYR_PAD * c;
    }
    size_t bytes;
    PyrDev dev;
    // Scharr derivative levels (what cv::calcOpticalFlowPyrLK materialises per call for its first image):
    // packed (4 dx & 0xffff) | (4 dy << 16) per pixel and channel (times 4: lk.hip), every level with a ZERO border of
    // SVO_DERIV_PAD pixels (the reference pads its derivative buffer with zeros) and a 16-byte-aligned
    // pitch.  Filled when the levels are built if want_deriv; LK needs them for its FIRST pyramid only.
    int *dbase = nullptr;
    size_t doff[SVO_MAX_LEVELS] = {0, 0, 0, 0};  // in ints: element (0, 0) of each level
    int dpitch[SVO_MAX_LEVELS] = {0, 0, 0, 0};   // bytes
    // grey storage (c == 3): offsets in `base` of the grey levels' padded buffers, and element (0, 0) of the grey
    // derivative levels in `dbase` (in ints)
    size_t goff[SVO_MAX_LEVELS] = {0, 0, 0, 0}, gdoff[SVO_MAX_LEVELS] = {0, 0, 0, 0};
    int gdelta[SVO_MAX_LEVELS] = {0, 0, 0, 0};  // bytes from origin(l) to pixel (0, 0) of grey level l
    bool want_deriv = true, has_deriv = false;
};
#define SVO_DERIV_PAD 32
int svo_build_derivatives(svo_ctx *ctx, int k, svo_pyramid *const *pyrs);
// lk.hip: a grey-stored pyramid's three-channel levels (and derivative levels) for the read-backs
int svo_expand_grey_storage(svo_ctx *ctx, const svo_pyramid *pyr, bool deriv);
int svo_pyramid_create_ex(svo_ctx *ctx, int width, int height, int channels, int levels, bool want_deriv,
                          svo_pyramid **out);

// growable device scratch
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes);
    void release();
    template <class T> T *as() { return reinterpret_cast<T *>(p); }
};

struct KernelTimer {
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pool;
    double total_ms = 0;
    int launches = 0;
};

struct svo_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool timing = false;
    KernelTimer timers[SVO_K_COUNT];
    // staging buffers for SVO_MEM_HOST calls
    DevBuf s_img, s_a, s_b, s_c, s_d, s_e, s_f, s_g;
    // work buffers used inside multi-kernel entry points
    DevBuf w_a, w_b, w_c, w_d, w_e;
    // SVO_N_TICKETS zeroed counters for "last workgroup finishes the job" kernels (self-resetting): 0..15 fransac.hip,
    // 16..31 pnp.hip, 32.. lk.hip (lk_expand_kernel: one per job and image of a tracking launch)
    unsigned *d_tickets = nullptr;
    void *pinned = nullptr;  // small pinned host block for scalar read-backs
    size_t pinned_bytes = 0;
    hipEvent_t wait_ev = nullptr;  // svo_wait(): event polled by the host
    // svo_orb_extract's extractor (work buffers, grey pyramid) and output staging, kept between calls of the same shape
    // (round 4: a call used to build and free them -- 1 ms per frame of allocation around 0.3 ms of kernels)
    struct svo_orb *orb_cache = nullptr;
    int orb_key[5] = {0, 0, 0, 0, 0};  // w, h, c, n_features, fast threshold
    DevBuf orb_out;
    std::vector<unsigned char> orb_host;  // svo_orb_extract with host outputs: the record block lands here
    // svo_orb_extract_batch's extractor in cv::ORB's shape (orb_cv.hip), kept between calls of the same shape; the sampling
    // pattern set through svo_orb_set_pattern (has_pattern: 0 = the seeded default)
    struct svo_orb_cv *orb_cv_cache = nullptr;
    int orb_cv_key[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // w, h, c, n_features, fast threshold, levels, scale factor bits, batch
    int8_t orb_pattern[1024];
    int has_pattern = 0;
    DevBuf orb_cv_out, orb_cv_img, orb_cv_ptrs;
    // host images in a lock-step group (frontend_chain.hip, chain_enqueue_lockstep): a copy stream of its own and a ring of three device
    // slots, each holding one step's left and right images of every chunk of the group -- step f + 2 is uploaded while
    // step f computes; up_ev: a slot's upload has landed, use_ev: its pyramids have been built
    hipStream_t up_stream = nullptr;
    DevBuf up_ring;
    hipEvent_t up_ev[3] = {nullptr, nullptr, nullptr}, use_ev[3] = {nullptr, nullptr, nullptr};
    // sgbm.hip: the dense matcher's cost volume and path planes, its per-pixel work arrays, the reprojection's staging
    DevBuf sgbm_cost, sgbm_misc, sgbm_rp;
    // bm.hip: the pre-filtered images, the per-pixel minimum SAD and the speckle filter's arrays (layout: bm_plan.hip.h)
    DevBuf bm_work;
    // sor_grid.hip: the large-cloud outlier removal's keys, sorted points, boxes and radix histograms
    DevBuf sor_grid;
    // cloud.hip: the staged source, the moved source in double, correspondences, partial sums and device states of one
    // registration call
    DevBuf icp_work;
    // essential.hip: normalised points, the RANSAC's per-iteration models / counts / state, recoverPose's candidate masks
    // (homography.hip's calls lay out the same buffer anew for their own models / counts / state / candidate masks)
    DevBuf ess;
    // sift.hip, brief.hip, surf.hip (feature_batch.hip.h, integral_scan.hip.h): the staged host images of a call (or surf.hip's
    // gathered grey device images), and the integral images of a batch with surf.hip's grey planes behind them.  One of each for
    // the three modules: every call fills them anew on the context's one stream, and DevBuf::ensure only ever grows a buffer
    DevBuf feat_img, feat_sum;
    // sift.hip: the scale space (Gaussian and DoG layers of every image of a batch), the detector's work arrays and key points,
    // the output block of host calls
    DevBuf sift_pyr, sift_work, sift_out;
    // brief.hip: the filter's and the descriptor kernel's work arrays, the test tables on the device (three slots of 2048 bytes:
    // 16 / 32 / 64-byte descriptors); brief_pattern: the tables set through svo_brief_set_pattern (brief_has_pattern[k] == 0: the
    // default), brief_pat_live[k]: slot k of brief_pat holds the current table
    DevBuf brief_work, brief_pat;
    int8_t brief_pattern[3][2048];
    int brief_has_pattern[3] = {0, 0, 0};
    int brief_pat_live[3] = {0, 0, 0};
    // surf.hip: the det / trace planes of every layer, the detector's candidate lists with the staged outputs of host calls
    DevBuf surf_planes, surf_work;
    // wls.hip: the filter's float planes, the two matchers' maps with the filtered map / confidence / grey guide behind them, and
    // the weight table on the device with the sigma and channel count it was built for (wls_lut_c == 0: none yet)
    DevBuf wls_work, wls_maps, wls_lut;
    std::vector<float> wls_lut_host;
    double wls_lut_sigma = 0;
    int wls_lut_c = 0;
    // fast.hip: the grey, fired and score planes of a batch, the per-wavefront counts and offsets of the ordered compaction, the
    // key-point lists of host calls and of the chained ANMS (layout: fast_plan.hip.h)
    DevBuf fast_work;
    // gftt.hip: the measure planes of a batch, the candidate keys and the sort's ping-pong arrays, the cell lists and states of the
    // selection, the staged masks and the corner lists of host calls (layout: gftt_plan.hip.h)
    DevBuf gftt_work;
    // voxel.hip: the keys, the sort's ping-pong arrays and histograms, the rows gathered in voxel order and the segment
    // starts (layout: voxel_plan.hip.h); voxel_stage: the inputs and outputs of a host call
    DevBuf voxel_work, voxel_stage;
    // rectify.hip: the images, maps and points of a host call (layout: rectify_plan.hip.h)
    DevBuf rect_stage;
    // ba_window.hip: the host copy of a device caller's CSR arrays, which the refusals are decided on
    std::vector<unsigned char> ba_win_host;
};

// Low-latency host wait for everything queued on the context's stream: records an event and
// polls it (hipStreamSynchronize parks the thread and costs tens of microseconds to wake).
int svo_wait(svo_ctx *ctx);
int svo_wait_stream(svo_ctx *ctx, hipStream_t stream);

// scoped timer: records events around a kernel when ctx->timing is on
struct ScopedKernelTime {
    svo_ctx *ctx;
    int id;
    hipEvent_t a = nullptr, b = nullptr;
    ScopedKernelTime(svo_ctx *c, int kid);
    ~ScopedKernelTime();
};
int svo_resolve_timers(svo_ctx *ctx);

// ---- the front-end's device-resident frame state (frontend_chain.hip: the chain runner) --------------------------------
// A chunk of frames is queued WITHOUT the host in the loop: the decisions the reference's host policy takes per
// frame -- keyframe iff fewer than 200 PnP inliers (src/VisualSLAM.cpp:120), retry / shutdown below 10
// (src/keyFrameManagement.cpp:85-92) -- are taken by pnp_finish_kernel and left here; the keyframe path's kernels are
// queued for EVERY frame and leave at once unless `kf` is set, every kernel leaves at once after a halt.
enum { SVO_HALT_NONE = 0, SVO_HALT_RETRY = 1 /* < pnp_retry_below inliers at 1 px: the host runs the 8 px retry */,
       SVO_HALT_FEW_REF = 2 /* fewer than 5 reference points for the next frame */ };
struct VoOut {  // one per frame of a run, in pinned host memory (what svo_vo_run_chunk returns per frame)
    double R[9], t[3];
    int inliers, tracked, keyframe, pad;
};
struct VoChain {
    // state, written by kernels
    int run;        // 1 while the chain is live; 0 after a halt
    int kf;         // 1: the frame just localised is a keyframe, its stereo path runs (implies run)
    int nref;       // live count of the reference set (ref2d / ref3d)
    int frame;      // frames of this run finished = index of the next one
    int halt_code;  // SVO_HALT_*
    int kf_n;       // points of the last keyframe's camera-frame cloud
    int refine_due; // 1: the frame's policy is decided, its refinement is left to a PNP_FINISH_REFINE launch
    int pad;
    double R[9], t[3];  // pose of the frame just localised, camera in world: the keyframe's [R|t]
    // configuration, written by the host before a run
    int kf_min, retry_below;
    float *ref2d, *ref3d;        // hand-over destination (src/VisualSLAM.cpp:143-146); the source is the PnP job's sets
    VoOut *out;                  // pinned host array, one record per frame of the run
};

// pyramid.hip
int svo_build_pyramid_from_device(svo_ctx *ctx, svo_pyramid *pyr, const uint8_t *d_image);
// gates (optional, one per pyramid): a pyramid whose *gate == 0 is left untouched (chain runner after a halt)
int svo_build_pyramids_from_device(svo_ctx *ctx, int k, svo_pyramid *const *pyrs, const uint8_t *const *d_images,
                                   const int *const *gates = nullptr);
// lk.hip
struct LkJob {  // one pyramidal-LK pass: prev/next pyramids, points in, points / status / err / minEig out
    PyrDev prev, next;
    const int *dprev;  // derivative levels of prev (svo_pyramid::dbase); geometry: svo_pyramid::doff / dpitch
    const float *prev_pts;
    int n_cap;
    const int *d_n;  // live point count on the device, or null (n_cap points)
    float *next_pts;
    uint8_t *status;
    float *err, *min_eig;  // optional
    const int *gate = nullptr;  // optional: the job's workgroups leave at once when *gate == 0 (VoChain::run / ::kf)
};
// NJ: SVO_LK_MAX_JOBS for the lock-step groups, 1 for a chunk on its own -- a launch of one job carries a sixteenth of the
// kernel arguments (the runtime stalls the launching thread for tens of microseconds per few hundred KB of them)
template <int NJ> struct LkBatchN {
    LkJob j[NJ];
};
using LkBatch = LkBatchN<SVO_LK_MAX_JOBS>;
// `geom`: any pyramid with the geometry of the jobs' prev pyramids (derivative level offsets / pitches)
int svo_launch_lk_batch(svo_ctx *ctx, int n_jobs, const LkJob *jobs, const svo_pyramid *geom);
int svo_launch_lk(svo_ctx *ctx, svo_pyramid *prev, const svo_pyramid *next, const float *prev_pts,
                  int n, float *next_pts, uint8_t *status, float *err, float *min_eig,
                  const int *d_n = nullptr);
int svo_launch_grid(svo_ctx *ctx, int rows, int cols, int step, float *out_xy, int cap);

// fransac.hip
struct svo_compact_job {  // order-preserving compaction of up to three float arrays by one byte mask
    const uint8_t *mask;
    int cap;
    const int *d_n;
    const float *in[3];
    float *out[3];
    int stride[3];
    int *d_count;
    const int *gate = nullptr;  // optional: leave at once when *gate == 0
    // optional: when *alt_sel != 0 the mask, the count and the input arrays given here replace the ones above (pipelined
    // chunk: the sets of the tracking pass from a keyframe's points rather than of the pass from the tracked set);
    // a null alt_in[k] / alt_d_n keeps the regular one
    const int *alt_sel = nullptr;
    const uint8_t *alt_mask = nullptr;
    const float *alt_in[3] = {nullptr, nullptr, nullptr};
    const int *alt_d_n = nullptr;
};
struct svo_fransac_job {  // host-side description of one F-matrix RANSAC problem (device pointers)
    const float *p1, *p2;
    int cap;
    const int *d_n;
    double threshold, confidence;
    int max_iters;
    uint64_t seed;
    uint8_t *mask;
    double *d_F;
    int *d_count, *d_iters;
    // optional: the compaction by the fresh mask (mask / cap / d_n of this job are used, the struct's own are
    // ignored), done by the waves that write the mask -- no launch of its own; the outputs must not overlap the inputs
    const svo_compact_job *then_compact = nullptr;
    const int *gate = nullptr;  // optional: every wave leaves at once when *gate == 0
    int gate_stride = 0;        // diagnostics only (svo_selftest_fransac_gate): workgroup b reads gate[b * gate_stride]
    // cv::findFundamentalMat's behaviour below 15 pairs (7: the solver once, mask all ones; 8..14: least median).  Off for the
    // loop detector's geometric check, whose upstream (DVision::FSolver) is a RANSAC at any count.
    bool cv_small = true;
};
int svo_launch_fransac_batch(svo_ctx *ctx, int n_jobs, const svo_fransac_job *jobs);
int svo_launch_fransac(svo_ctx *ctx, const float *p1, const float *p2, int cap, const int *d_n,
                       double threshold, double confidence, int max_iters, uint64_t seed, uint8_t *mask,
                       double *d_F, int *d_count, int *d_iters, const svo_compact_job *then_compact = nullptr,
                       bool cv_small = true);
int svo_fransac_ex(svo_ctx *ctx, const float *p1, const float *p2, int n, double threshold, double confidence, int max_iters,
                   uint64_t seed, uint8_t *mask, double *F9, int *inlier_count, int *iters_run, int mem, bool cv_small);
// geometry.hip
int svo_launch_triangulate(svo_ctx *ctx, const double *P1, const double *P2, const float *x1, const float *x2,
                           int cap, const int *d_n, float *out_xyz, float *out_h, const double *Rt,
                           float *out_world);
struct svo_tri_job {  // one stereo DLT triangulation (device pointers; Rt: host 3x4 or null)
    const float *x1, *x2;
    int cap;
    const int *d_n;
    float *out_xyz, *out_h;
    const double *Rt;
    float *out_world;
    int *h_count;  // pinned host int that receives the live count, or null
    // chain mode (optional): [R|t] is read from chain->R / chain->t on the device (Rt must be null), the job runs only
    // when chain->kf is set, the live count goes to chain->nref / chain->kf_n and fewer than 5 points halt the chain
    VoChain *chain = nullptr;
    float *out_x1 = nullptr;  // optional: a copy of x1 (the keyframe's 2-D reference set when x1 is a staging buffer)
    // optional: getColors(imL, x1) -- img.at<Vec3b>(int(y), int(x)) as 3 floats (include/monoUtils.h:180-193), the
    // `colors` member stereoTriangulate fills at src/triangulation.cpp:139-140 -- gathered by the same kernel
    const svo_pyramid *color_src = nullptr;
    float *color_out = nullptr;
};
int svo_launch_triangulate_batch(svo_ctx *ctx, const double *P1, const double *P2, int k, const svo_tri_job *jobs);
// a keyframe whose camera-frame points were triangulated ahead of the decision: the chain-mode tail of the triangulation
// launch alone (runs only when chain->kf is set; [R|t] from the chain state).  what: 1 = the pose-free part (set size,
// 2-D set, colours), 2 = the clouds (camera frame, and placed with the pose), 3 = both
int svo_launch_keyframe_place(svo_ctx *ctx, VoChain *chain, const float *x1, const float *xyz, int cap, const int *d_n,
                              float *out_x1, float *out_cam, float *out_world, const svo_pyramid *color_src, float *color_out,
                              int what);
int svo_launch_transform(svo_ctx *ctx, const double *Rt, const float *in, int cap, const int *d_n, float *out);
int svo_launch_colors(svo_ctx *ctx, const svo_pyramid *pyr, const float *xy, int cap, const int *d_n, float *out);
int svo_launch_compact_batch(svo_ctx *ctx, int n_jobs, const svo_compact_job *jobs);
int svo_launch_compact(svo_ctx *ctx, const uint8_t *mask, int cap, const int *d_n, const float *in_a, int stride_a,
                       float *out_a, const float *in_b, int stride_b, float *out_b, const float *in_c, int stride_c,
                       float *out_c, int *d_count);
// orb.hip -- features of the loop-closure detector
struct svo_orb;
int svo_orb_create(svo_ctx *ctx, int w, int h, int c, int n_features, int fast_t, svo_orb **out);
int svo_orb_destroy(svo_orb *o);
int svo_orb_launch(svo_orb *o, const uint8_t *d_image, float *d_xy, int *d_oct, float *d_resp, float *d_dir,
                   uint32_t *d_desc, int *d_n);
// orb_cv.hip -- the same in cv::ORB's own shape (n levels x scale factor, settable pattern), up to 32 images per launch
struct svo_orb_cv;
int svo_orb_cv_create(svo_ctx *ctx, int w, int h, int c, int n_features, int fast_t, int n_levels, float scale_factor, int batch,
                      const int8_t *pattern, svo_orb_cv **out);
int svo_orb_cv_destroy(svo_orb_cv *o);
int svo_orb_cv_set_pattern(svo_orb_cv *o, const int8_t *pattern);
int svo_orb_cv_batch(const svo_orb_cv *o);
int svo_orb_cv_launch(svo_orb_cv *o, const uint8_t *const *d_images, int n_images, int cap_out, float *d_xy, int *d_oct,
                      float *d_resp, float *d_dir, uint32_t *d_desc, int *d_n, hipStream_t st);
void svo_orb_default_pattern(int8_t *pat);
// sgbm.hip: filterSpeckles(disp, new_val, max_size, max_diff) in place on n_pairs maps of h x w, back to back on the device;
// parent / sizes: n_pairs * w * h ints each
int svo_launch_speckle(hipStream_t st, int16_t *disp, int *parent, int *sizes, int w, int h, int n_pairs, int new_val,
                       int max_diff, int max_size);
// sor.hip
int svo_launch_sor(svo_ctx *ctx, const float *xyz, const float *color, int cap, int mean_k, double stddev_mul,
                   float z_limit, float *xyz_out, float *color_out, int *d_count, float *d_mean_dist, int *d_pass);
// sor_grid.hip: the same contract for up to 2^22 points (Morton sort + box hierarchy kNN); mean_k 1..256
int svo_launch_sor_large(svo_ctx *ctx, const float *xyz, const float *color, int cap, int mean_k, double stddev_mul,
                         float z_limit, float *xyz_out, float *color_out, int *d_count, float *d_mean_dist, int *d_pass);
// pnp.hip
struct svo_pnp_job {  // host-side description of one PnP-RANSAC problem (device pointers)
    const float *obj, *img;
    int cap;
    const int *d_n;
    double K4[4];
    int iterations;
    double reproj_err, confidence;
    uint64_t seed;
    int refine_iters;
    int *inliers;
    uint8_t *mask;
    void *d_result;
    // optional: chain mode -- the policy of the frame is decided on the device (see VoChain): inlier count against
    // chain->retry_below / chain->kf_min, pose composition (src/VisualSLAM.cpp:70-74), the per-frame record into
    // chain->out[chain->frame], the reference hand-over when the frame is no keyframe; the job's kernels leave at
    // once when chain->run == 0
    VoChain *chain = nullptr;
    const int *cnt_trk;
};
// split: the finishing launch is queued as PNP_FINISH_DECIDE, the refinement is left to svo_launch_pnp_refine (chain
// jobs only; the caller queues it on another stream: once for keyframes, before their cloud is placed, once for the
// other frames, beside whatever follows)
int svo_launch_pnp_ransac_batch(svo_ctx *ctx, int n_jobs, const svo_pnp_job *jobs, bool split);
int svo_launch_pnp_refine(svo_ctx *ctx, int n_jobs, const svo_pnp_job *jobs, bool keyframes);
int svo_launch_pnp_ransac_batch(svo_ctx *ctx, int n_jobs, const svo_pnp_job *jobs);
int svo_launch_pnp_ransac(svo_ctx *ctx, const float *obj, const float *img, int cap, const int *d_n,
                          const double *K4h, int iterations, double reproj_err, double confidence, uint64_t seed,
                          int refine_iters, int *inliers, uint8_t *mask, void *d_result);
int svo_launch_solve_pnp(svo_ctx *ctx, const float *obj, const float *img, int cap, const int *d_n, const double *K4h,
                         int refine_iters, int *inliers, void *d_result);
// anms.hip
// optional gather of the kept keypoints in the same launch that lists them (out_x[i] = in_x[out_idx[i]])
struct svo_anms_gather {
    const float *in_a, *in_b;  // float2 arrays
    float *out_a, *out_b;
    const uint8_t *in_s;
    uint8_t *out_s;
};
// gates (optional): per job, the job's workgroups leave at once when *gates[a] == 0
int svo_launch_anms_batch(svo_ctx *ctx, int k, const float *const *xy, const float *const *resp, int n, int keep,
                          int *const *out_idx, int *const *d_count, const svo_anms_gather *gather = nullptr,
                          const int *const *gates = nullptr);
int svo_launch_anms(svo_ctx *ctx, const float *xy, const float *resp, int n, int keep, int *out_idx, int *d_count);

// ---- png.hip: PNG decoding for the sequence reader (host code); NULL = ok, else the reason ----
const char *svo_png_info(const uint8_t *data, size_t n, int *w, int *h, int *c);
const char *svo_png_decode(const uint8_t *data, size_t n, int channels, uint8_t *out, size_t cap, int *w, int *h);

// ---- bow.hip: the vocabulary tree and the bag-of-words database kernels (used by loopdet.hip) --------------------------
struct svo_voc;
constexpr int SVO_LC_MAX_CAND = 64;
struct svo_lc_bow_record {  // what the host logic of detectLoop reads for one frame, in pinned memory
    int ready;       // entry id + 1 once the record is complete (released at system scope)
    int nq;          // words of the query's BowVector
    int n_cand, n_feat;  // n_feat: features of the frame
    double last_sum;                      // raw L1 sum against entry id - 1 (the normalisation score is -last_sum / 2)
    int cand_id[SVO_LC_MAX_CAND];         // best first: sum ascending (= score descending), entry id ascending on ties
    double cand_sum[SVO_LC_MAX_CAND];
};
// n_frames > 1: the frames of a batch (svo_lc_submit_batch) -- `cap` slots per frame in every array, consecutive database
// rows / records, one count per frame
int svo_voc_launch_transform(svo_voc *v, hipStream_t st, const uint32_t *d_desc, int cap, const int *d_n, int levelsup,
                             int *d_word, double *d_weight, int *d_node, int n_frames = 1);
int svo_bow_launch_vector(hipStream_t st, const int *d_word, const double *d_weight, const int *d_node, int cap, const int *d_n,
                          int *row_w, double *row_v, int *row_n, int *row_node, int n_frames = 1);
int svo_bow_launch_query(hipStream_t st, const int *qw, const double *qv, const int *d_nq, int nf, const int *head,
                         const int *next, const double *db_v, int stride, int n_entries, double *plane, int pitch, double *sums,
                         int dislocal, int k_want, int entry_id, const int *d_nfeat, svo_lc_bow_record *rec, int n_frames, unsigned *mask);
// mask: n_frames x pitch x svo_bow_mask_words(nf) words, ZERO before the first query (the query leaves it zero): which rows of an
// entry's column of the plane hold a term of the current query
inline int svo_bow_mask_words(int nf) { return ((nf + 127) / 128) * 4; }
int svo_bow_launch_link(hipStream_t st, const int *row_w, const int *row_n, int nf, int slot0, int *head, int *next, int n_frames = 1);
// the direct-index matching of up to SVO_LK_MAX_JOBS geometric checks in one launch (loopdet.hip: a look-ahead group): check s
// compares database entries old_entry[s] (na[s] features) and cur_entry[s]; [best_j | d1 | d2] (3 nf ints) go to out + s * out_stride
struct SvoDiBatch {
    int old_entry[SVO_LK_MAX_JOBS], cur_entry[SVO_LK_MAX_JOBS], na[SVO_LK_MAX_JOBS];
};
int svo_bow_launch_di_nearest_batch(hipStream_t st, const SvoDiBatch &b, int n_checks, int na_max, const uint32_t *db_desc,
                                    const int *db_node, const int *db_n, int nf, uint8_t *out, size_t out_stride);
int svo_bow_launch_di_nearest(hipStream_t st, const uint32_t *A, const int *node_a, int na, const uint32_t *B, const int *node_b,
                              const int *d_nb, int *best_j, int *d1, int *d2);
int svo_voc_words_internal(const svo_voc *v);
int svo_voc_device_internal(const svo_voc *v);
int svo_voc_levels_internal(const svo_voc *v);
