/*
 * svo.h -- C ABI of libsvo_hip.so: the MI355X (gfx950) stereo-VO + pose-graph hot path.
 *
 * This is the drop-in boundary for the hot path of Gautham-JS/ROS_Stereo_SLAM.  The
 * reference has no FFI of its own: its hot path is the member surface of
 * include/visualSLAM.h:152-178 and include/poseGraph.h:62-66, which call straight into
 * OpenCV and g2o.  Each entry point below names the reference interface it replaces
 * (file:line relative to the reference checkout).  The C++ adaptors in
 * include/svo_compat/ rebuild the reference's member functions on top of this ABI;
 * INTEGRATION.md shows the binding a maintainer adds.
 *
 * Conventions
 *  - plain pointers and sizes, no C++ or torch types; every function returns an int
 *    status (SVO_OK == 0, negative = error; svo_last_error() holds the text).
 *  - `mem` says where the caller's arrays live: SVO_MEM_HOST (the library stages through
 *    its own device scratch and synchronises before returning) or SVO_MEM_DEVICE (HBM
 *    pointers on the context's device; work is queued on the context's stream and the
 *    call returns without synchronising -- use svo_ctx_sync()).
 *  - one svo_ctx per device; it owns the HIP stream, scratch buffers and kernel timers.
 *    No global state.  A context is not re-entrant (the reference is single-threaded on
 *    this path too: src/VisualSLAM.cpp:54-200 runs on the main thread).
 *  - images: H x W x C uint8, interleaved channels, row stride W*C (cv::Mat CV_8UC3
 *    continuous, as src/keyFrameManagement.cpp:48-71 loads them).  Points: float32 x,y
 *    (cv::Point2f) / x,y,z (cv::Point3f).  Camera matrices, rvec/tvec, [R|t]: float64.
 *  - there is NO CPU fallback: without a gfx950 device svo_ctx_create() fails with
 *    SVO_ERR_NO_DEVICE and nothing else can be called.
 */
#ifndef SVO_H
#define SVO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SVO_VERSION 100

enum {
    SVO_OK = 0,
    SVO_ERR_ARG = -1,
    SVO_ERR_HIP = -2,
    SVO_ERR_CAPACITY = -3,
    SVO_ERR_NO_DEVICE = -4,
    SVO_ERR_TRACKING_LOST = -5, /* the reference's SHUTDOWN_FLAG, keyFrameManagement.cpp:89-92 */
    SVO_ERR_STATE = -6
};
enum { SVO_MEM_HOST = 0, SVO_MEM_DEVICE = 1 };

/* kernel ids for svo_ctx_kernel_time() */
enum {
    SVO_K_PYRAMID = 0,
    SVO_K_LK = 1,
    SVO_K_FRANSAC = 2,
    SVO_K_TRIANGULATE = 3,
    SVO_K_PNP = 4,
    SVO_K_POSEGRAPH = 5,
    SVO_K_ANMS = 6,
    SVO_K_BRIEF_INTEGRAL = 7, /* svo_brief_*: the row and column passes of the integral images */
    SVO_K_BRIEF_DESCRIBE = 8, /* svo_brief_describe_batch: the key-point filter and the descriptor kernel */
    SVO_K_COUNT = 9
};

typedef struct svo_ctx svo_ctx;
typedef struct svo_pyramid svo_pyramid;
typedef struct svo_vo svo_vo;
typedef struct svo_posegraph svo_posegraph;

int svo_version(void);
const char *svo_last_error(void);

/* ---- context ----------------------------------------------------------------------------- */
int svo_ctx_create(int device, svo_ctx **out);
int svo_ctx_destroy(svo_ctx *ctx);
int svo_ctx_sync(svo_ctx *ctx);
/* the hipStream_t all work of this context is queued on */
void *svo_ctx_stream(svo_ctx *ctx);
/* per-kernel HIP-event timing on the context's stream (bench.py's roofline leg) */
int svo_ctx_enable_kernel_timing(svo_ctx *ctx, int enable);
int svo_ctx_kernel_time(svo_ctx *ctx, int kernel_id, double *total_ms, int *launches);
int svo_ctx_reset_kernel_time(svo_ctx *ctx);

/* ---- shared transcendental functions (include/svo_math.h) ------------------------------------
 * The geometry solvers on both sides of the parity tests call ONE software implementation of sin /
 * cos / acos / cbrt / log (the reference reaches libm through OpenCV: Rodrigues at
 * src/VisualSLAM.cpp:71, the cubic of findFundamentalMat at src/tracking.cpp:34,75, the adaptive
 * RANSAC bound of solvePnPRansac at src/keyFrameManagement.cpp:84).  This entry evaluates one of them
 * ON THE DEVICE over an array, so that a test can check the device and the host run it bit for bit. */
enum { SVO_MATH_SIN = 0, SVO_MATH_COS = 1, SVO_MATH_ACOS = 2, SVO_MATH_CBRT = 3, SVO_MATH_LOG = 4, SVO_MATH_EXP = 5 };
int svo_math_eval(svo_ctx *ctx, int fn, const double *x, int n, double *y, int mem);

/* ---- diagnostics ---------------------------------------------------------------------------
 * svo_selftest_fransac_gate: ONE findFundamentalMat launch sequence (src/tracking.cpp:34) in which the workgroups of
 * every launch DISAGREE about the chunk runner's launch gate (even workgroups see it open, odd ones closed) -- the view
 * a pipelined chunk can produce when the PnP stream halts the chain under a launch another stream is dispatching.
 * tickets_after[0..1] receive the "last workgroup finishes" counters of the context afterwards; they must be 0, and the
 * next ordinary svo_fransac on the context must give its usual answer.  Device pointers; lean != 0: the single-wave
 * build the lock-step groups use (two jobs), else the lone-chunk build.  The mask's contents are unspecified. */
int svo_selftest_fransac_gate(svo_ctx *ctx, const float *d_p1, const float *d_p2, int n, double threshold,
                              uint64_t seed, int lean, uint8_t *d_mask, unsigned *tickets_after);
/* svo_selftest_scan: the workgroup prefix scan under every ordered compaction of the library (csrc/scan_ops.hip.h), run by
 * ONE workgroup: d_out[0..n) = the exclusive prefix sums of d_in[0..n), *d_total = the sum.  kind selects the workgroup size
 * and the element type.  Device pointers of that type; d_out == d_in is allowed; n <= 2^24.  Returns after the launch has
 * finished. */
enum { SVO_SCAN_256_INT = 0, SVO_SCAN_1024_UINT = 1, SVO_SCAN_1024_U64 = 2 };
int svo_selftest_scan(svo_ctx *ctx, int kind, const void *d_in, int n, void *d_out, void *d_total);

/* ---- image pyramid ----------------------------------------------------------------------- */
/* Replaces the pyramid cv::calcOpticalFlowPyrLK rebuilds on every call
 * (src/tracking.cpp:18,52).  A pyramid is built once per image and reused for the
 * (t-1 -> t), (t -> t+1) and (left -> right) trackings that read it.                       */
int svo_pyramid_create(svo_ctx *ctx, int width, int height, int channels, int levels,
                       svo_pyramid **out);
int svo_pyramid_destroy(svo_ctx *ctx, svo_pyramid *pyr);
int svo_pyramid_build(svo_ctx *ctx, svo_pyramid *pyr, const uint8_t *image, int mem);
/* *out = 1 when the image the pyramid was last built from has B == G == R in every pixel (3-channel pyramids only;
 * 1- and 4-channel pyramids and pyramids never built say 0): the word the build leaves on the device for the tracker,
 * which then sums one channel of a grey frame stored as BGR.  Read back in stream order (tests and tools). */
int svo_pyramid_is_mono(svo_ctx *ctx, const svo_pyramid *pyr, int *out);
/* copy one level out (tests).  out holds w*h*c bytes. */
int svo_pyramid_get_level(svo_ctx *ctx, const svo_pyramid *pyr, int level, uint8_t *out,
                          int mem, int *w, int *h);
/* svo_pyramid_create with the choice of derivative levels: want_deriv == 0 makes a pyramid that carries none (a right
 * image, never the first image of a tracking pass).  svo_lk_track derives them on demand when such a pyramid does become
 * its first image, and again after every later build. */
int svo_pyramid_create2(svo_ctx *ctx, int width, int height, int channels, int levels, int want_deriv,
                        svo_pyramid **out);
/* copy one level out AS STORED, with its reflect-101 border of 32 pixels on every side (tests): rows are packed,
 * out holds (h + 64) * (w + 64) * c bytes; *pw and *ph receive the padded sizes.  out == NULL: the sizes only. */
int svo_pyramid_get_padded_level(svo_ctx *ctx, const svo_pyramid *pyr, int level, uint8_t *out, int mem,
                                 int *pw, int *ph);
/* copy one Scharr derivative level out as stored (tests): one int32 word (4 dx & 0xffff) | (4 dy << 16) per pixel and
 * channel, with its zero border of 32 pixels; rows are packed, out holds (h + 64) * (w + 64) * c words.  out == NULL: the
 * sizes only.  SVO_ERR_STATE when the pyramid holds no derivative levels at present (4 channels, created without them and
 * not yet a tracking pass's first image, or never built). */
int svo_pyramid_get_derivative_level(svo_ctx *ctx, const svo_pyramid *pyr, int level, int32_t *out, int mem,
                                     int *pw, int *ph);

/* ---- dense grid sampler: visualSLAM::denseKeypointExtractor, src/tracking.cpp:4-12 ------- */
int svo_grid_keypoints(svo_ctx *ctx, int rows, int cols, int step, float *out_xy, int cap,
                       int mem, int *count);

/* ---- pyramidal Lucas-Kanade: cv::calcOpticalFlowPyrLK with defaults ----------------------- */
/* replaces the calls at src/tracking.cpp:18 (denseLKtracking) and :52
 * (PyrLKtrackFrame2Frame).  21x21 window, 4 levels, 30 iterations / 0.01, minEig 1e-4.
 * err and min_eig may be NULL.  min_eig is the level-0 minimum eigenvalue (ANMS response). */
int svo_lk_track(svo_ctx *ctx, const svo_pyramid *prev, const svo_pyramid *next,
                 const float *prev_pts, int n, float *next_pts, uint8_t *status, float *err,
                 float *min_eig, int mem);

/* Up to 16 independent tracking passes of one geometry in ONE launch, as the lock-step front-ends queue them (device
 * pointers throughout, asynchronous on the context's stream).  d_err, d_min_eig, d_gates and their entries may be NULL;
 * a job whose *d_gates[a] == 0 writes nothing.  Tests and tools. */
int svo_lk_track_jobs(svo_ctx *ctx, int n_jobs, svo_pyramid *const *prev, const svo_pyramid *const *next,
                      const float *const *d_prev_pts, const int *n, float *const *d_next_pts, uint8_t *const *d_status,
                      float *const *d_err, float *const *d_min_eig, const int *const *d_gates);
/* svo_pyramid_build of a device image behind a gate, as the chain runner queues it: with *d_gate == 0 (a device int) the
 * pyramid is left as it was.  d_gate may be NULL.  Asynchronous on the context's stream. */
int svo_pyramid_build_gated(svo_ctx *ctx, svo_pyramid *pyr, const uint8_t *d_image, const int *d_gate);
/* k pyramids of ONE geometry (width, height, channels, levels) from k device images in one set of launches, as the
 * lock-step front-ends queue them: 1 <= k <= 32.  d_gates may be NULL; otherwise it holds k device int pointers, each of
 * which may be NULL, and pyramid a is left as it was when *d_gates[a] == 0.  Asynchronous on the context's stream. */
int svo_pyramid_build_many(svo_ctx *ctx, int k, svo_pyramid *const *pyrs, const uint8_t *const *d_images,
                           const int *const *d_gates);

/* ---- order-preserving compaction by a byte mask -------------------------------------------- */
/* replaces the push_back filters of src/tracking.cpp:20-27 (status), :35-42 and :66-84 (mask).
 * Up to three float arrays (a, b, c; stride = floats per element, NULL to skip) are compacted
 * with one mask; rows with mask == 1 are kept in order.  count: host int (SVO_MEM_HOST) or
 * device int (SVO_MEM_DEVICE).  Device outputs must not overlap the inputs (the segments of the
 * array are compacted by independent wavefronts).                                           */
int svo_compact(svo_ctx *ctx, const uint8_t *mask, int n, const float *in_a, int stride_a, float *out_a,
                const float *in_b, int stride_b, float *out_b, const float *in_c, int stride_c, float *out_c,
                int *count, int mem);

/* ---- fundamental-matrix RANSAC: cv::findFundamentalMat(p1,p2,FM_RANSAC,thr,conf,mask) ------ */
/* replaces src/tracking.cpp:34 (FmatThresholding: thr 3.0, conf 0.99) and :75
 * (PyrLKtrackFrame2Frame: method 8 == FM_RANSAC, thr 1.0, conf 0.99).  max_iters is OpenCV's
 * fixed 1000.  mask: n bytes (1 = inlier).  F9 (optional): the winning 7-point model, row
 * major, unit Frobenius norm.  inlier_count / iters_run (optional): host or device ints
 * following `mem`.  Sampling is a counter-based generator keyed by (seed, iteration).        */
int svo_fransac(svo_ctx *ctx, const float *p1, const float *p2, int n, double threshold,
                double confidence, int max_iters, uint64_t seed, uint8_t *mask, double *F9,
                int *inlier_count, int *iters_run, int mem);
/* The batch form the lock-step front-ends queue: 1 <= k <= 16 independent problems in ONE launch sequence, with the
 * order-preserving compaction of up to three payload arrays by each fresh mask riding along (no launch of its own).
 * DEVICE pointers throughout, asynchronous on the context's stream.  Two problems or more run the single-wave build, one
 * problem the lone-chunk build svo_fransac runs.
 *   cap        capacity of p1 / p2 / mask / payload; the mask's cap bytes are all written (zero from the live count on)
 *   d_n        live count (device int, clamped to cap), or NULL: cap pairs
 *   F9, inlier_count, iters_run   optional, as in svo_fransac
 *   payload_in[a] / payload_out[a] / payload_stride[a]   rows of payload_stride[a] floats, cap of them; the rows with
 *              mask == 1 go to payload_out[a] in order.  payload_in[0] == NULL: no compaction.  Outputs must not overlap
 *              inputs.  payload_count (optional): the number of rows kept
 *   gate       optional device int: with *gate == 0 the problem's outputs are left untouched */
typedef struct svo_fransac_problem {
    const float *p1, *p2;
    int cap;
    const int *d_n;
    double threshold, confidence;
    int max_iters;
    uint64_t seed;
    uint8_t *mask;
    double *F9;
    int *inlier_count, *iters_run;
    const float *payload_in[3];
    float *payload_out[3];
    int payload_stride[3];
    int *payload_count;
    const int *gate;
} svo_fransac_problem;
int svo_fransac_batch(svo_ctx *ctx, int k, const svo_fransac_problem *problems);

/* ---- stereo triangulation: src/triangulation.cpp:142-160 ------------------------------------ */
/* P1 = K[I|0], P2 = K[I|(-b,0,0)^T] (3x4 row-major doubles, HOST memory always). */
int svo_stereo_projections(double fx, double fy, double cx, double cy, double baseline, double *P1,
                           double *P2);
/* cv::triangulatePoints + float dehomogenisation.  out_xyz: n*3 floats; out_h4 (optional): the
 * unit-norm homogeneous vectors (sign arbitrary).  P1/P2 are host pointers.                  */
int svo_triangulate(svo_ctx *ctx, const double *P1, const double *P2, const float *x1, const float *x2,
                    int n, float *out_xyz, float *out_h4, int mem);
/* visualSLAM::update3dtransformation / the loop of insertKeyFrames,
 * src/keyFrameManagement.cpp:20-30,33-46.  Rt: 3x4 row-major doubles in HOST memory.          */
int svo_transform_points(svo_ctx *ctx, const double *Rt, const float *in_xyz, int n, float *out_xyz,
                         int mem);
/* getColors, include/monoUtils.h:180-193: B,G,R of level 0 at (int(y), int(x)) as floats.      */
int svo_get_colors(svo_ctx *ctx, const svo_pyramid *pyr, const float *xy, int n, float *out_bgr, int mem);

/* ---- duplicate-aware replenishment of a tracked set: removeDuplicate and the top-up of trackSequence, src/ROSslam.py:156-169,
 * 262-271, and removeDuplicates, include/monoUtils.h:195-213 ----------------------------------------------
 * svo_dedup_points: keep[i] = 1 when new point i has no reference point near it, else 0.  xy arrays hold 2 floats per point.
 *   SVO_DEDUP_BOX   the prototype: i is a duplicate when some reference point has rx > qx - r && rx < qx + r && ry > qy - r &&
 *                   ry < qy + r, every operand promoted to double first (the prototype's query points are float64), all four
 *                   comparisons strict: |dx| == r is no duplicate.  The prototype marks a duplicate by zeroing the point and returns
 *                   "x != 0", so a new point whose own x is exactly 0 is dropped whether or not it has a neighbour; that artefact is
 *                   reproduced (keep = 0 for qx == 0, also with n_ref == 0).
 *   SVO_DEDUP_DISC  the C++ side: i is a duplicate when sqrt((double)dx * dx + (double)dy * dy) < radius, dx and dy the FLOAT
 *                   differences ref - new (Point2f::operator-), the sum of the two double products formed without contraction, the
 *                   double square root compared with <.  Squares are not compared: sqrt(s) < r and s < r * r differ when s is one
 *                   ulp below r * r.
 * ref_idx is the reference's `mask`: only the n_idx listed reference points take part, in any order, repeats allowed; an entry
 * outside [0, n_ref) is skipped and nothing is read through it.  ref_idx == NULL (n_idx must then be 0) means all n_ref points; a
 * non-null ref_idx with n_idx == 0 means none.  A NaN coordinate makes every comparison false: such a new point is kept, such a
 * reference point drops nobody.  n_keep (optional): the number of ones, a host or a device int following `mem`.  n_new == 0 and
 * n_ref == 0 are legal.  SVO_ERR_ARG, with nothing written: null ctx, a negative count, a radius that is negative or NaN, an unknown
 * mode or mem, n_idx != 0 with a null ref_idx, a null array whose count is not 0, a count above 2^28.
 *
 * svo_replenish: the loop body of src/ROSslam.py:262-271 without a host round trip.  The n_new new points are tested against
 * ref_xy[0 .. n_ref) as above; each survivor's 3-D point is moved with Rt (3 x 4 row-major HOST doubles; the arithmetic of
 * svo_transform_points: double products of the float input in the order x, y, z, t, rounded to float at the store) and kept when the z
 * of the STORED float is > 0; the kept points are appended in input order to ref_xy (2 floats a row) and ref_xyz (3 floats a row)
 * from row n_ref on.  Rows [0, n_ref) and rows past the new count are left as they were.  n_out = the new size, n_dup = points dropped
 * as duplicates, n_behind = points dropped for z <= 0 (a NaN z included): optional, host or device ints following `mem`;
 * n_dup + n_behind + (n_out - n_ref) == n_new.  cap = rows ref_xy / ref_xyz can hold; cap < n_ref + n_new is refused with
 * SVO_ERR_CAPACITY before anything is launched (the worst case is checked, so the device never overflows).  The result is, bit for
 * bit, svo_dedup_points -> svo_compact -> svo_transform_points -> a host z > 0 mask -> svo_compact -> concatenation.  In device
 * memory nothing waits for the device; the new arrays must not overlap the reference arrays.  The prototype keeps float64 points
 * (cv2.triangulatePoints on double input); these are float, as on the C++ path.                                                    */
#define SVO_DEDUP_BOX  0 /* src/ROSslam.py:156-169 */
#define SVO_DEDUP_DISC 1 /* include/monoUtils.h:195-213 */
int svo_dedup_points(svo_ctx *ctx, const float *ref_xy, int n_ref, const int *ref_idx, int n_idx, const float *new_xy,
                     int n_new, double radius, int mode, uint8_t *keep, int *n_keep, int mem);
int svo_replenish(svo_ctx *ctx, float *ref_xy, float *ref_xyz, int n_ref, int cap, const float *new_xy, const float *new_xyz,
                  int n_new, double radius, int mode, const double *Rt, int *n_out, int *n_dup, int *n_behind, int mem);

/* ---- map clean-up: visualSLAM::SORcloud(ref3d, colorMap), src/rosFuncs.cpp:9-39 ------------- */
/* Drops points with -z > z_limit (500 upstream, :12; <= 0 disables), then the statistical
 * outlier removal PCL applies at :19-23 (mean_k 200, stddev_mul 0.01): mean distance to the
 * mean_k nearest other points, keep d <= mean + stddev_mul * stddev.  xyz / color: n x 3 floats
 * (color may be NULL, then color_out is ignored); outputs compacted in input order, n capacity.
 * n_out / n_pass_out (points that passed the z filter, optional) are HOST ints in both modes;
 * mean_dist_out (optional, n floats): the mean neighbour distance of every point that passed the
 * z filter.  At most 9216 points per call.                                                     */
int svo_sor_filter(svo_ctx *ctx, const float *xyz, const float *color, int n, int mean_k, double stddev_mul,
                   float z_limit, float *xyz_out, float *color_out, int *n_out, float *mean_dist_out,
                   int *n_pass_out, int mem);
/* The same filter for large clouds -- StereoProcess::pclPublish's pcl::StatisticalOutlierRemoval (MeanK 20,
 * StddevMulThresh 0.8, src/StereoCV.cpp:289-293) of a dense cloud, or SORcloud of an accumulated map.  Same
 * arguments and outputs as svo_sor_filter, for n up to 4194304 (2^22, else SVO_ERR_CAPACITY) and mean_k 1..256
 * (else SVO_ERR_ARG).  For every cloud both accept it returns the same bits as svo_sor_filter: mean distances, kept
 * points and colours.  That holds because the multiset of the kk = min(mean_k, m - 1) smallest float squared
 * distances is unique (ties cannot change it), and its double sum of square roots does not depend on order whenever
 * it is exact (any realistic spread: exact while the largest term over the smallest nonzero one stays below
 * 2^29 / kk).  A point with a NaN or infinite coordinate is dropped with the z pre-filter: it counts neither as
 * passed nor as kept (PCL would keep it).  In device mode the outputs must not overlap the inputs.  The search is
 * an exact kNN over the Morton-sorted cloud with a box hierarchy.                        */
int svo_sor_filter_large(svo_ctx *ctx, const float *xyz, const float *color, int n, int mean_k, double stddev_mul,
                         float z_limit, float *xyz_out, float *color_out, int *n_out, float *mean_dist_out,
                         int *n_pass_out, int mem);

/* ---- voxel-grid down-sampling: Open3D's voxel_down_sample, the filter both clouds of the multiway-registration recipe pass
 * through before estimate_normals and registration_icp -- the recipe PoseGraphOptimize's downSampleFactor * 15 / * 1.5 come from,
 * src/ROSslam.py:34-40 (every recalled point and every choice of ours: tests/voxel_numpy.py) --------------
 * xyz / color: n x 3 floats, n in 0 ... 4194304 (2^22, else SVO_ERR_CAPACITY); color may be NULL, then color_out is ignored.
 *   1. A point with a NaN or infinite coordinate is dropped and takes part in nothing (svo_sor_filter_large's rule).
 *   2. min_bound[a] = (double)min_a - voxel_size * 0.5 over the remaining points.
 *   3. The cell of a point on axis a is (int64)floor(((double)p_a - min_bound[a]) / voxel_size): a double subtraction, a double
 *      division, floor; no reciprocal, no contraction.
 *   4. The key of a cell is (i_z << 42) | (i_y << 21) | i_x.  An axis that spans 2^21 cells or more (cells = the cell of the
 *      largest coordinate + 1, svo_voxel_grid) is refused with SVO_ERR_CAPACITY and nothing is written: Open3D's "voxel_size is
 *      too small".  It is decided on the host from the finite bounds before any key is formed; hence no index reaches 2^21.
 *   5. One output row per occupied cell, in ascending key order: per component the double sum of the cell's points, taken left
 *      to right in ascending input index, divided by (double)count and rounded to float at the store; colours likewise.
 *   6. point_voxel (optional, n ints): the output row of every input point, -1 for a dropped one.  voxel_count (optional): the
 *      points of every output row.
 * Every output has n rows of capacity; rows past *n_out are left as they were.  *n_out is a HOST int in both modes and the call
 * waits for it (and for the outputs).  In device mode the outputs must not overlap the inputs.  SVO_ERR_ARG, with nothing written:
 * a null ctx, n < 0, a voxel_size that is <= 0, NaN or infinite, an unknown mem, a null xyz, xyz_out or n_out with n > 0, a null
 * color_out with colours given.  n == 0 and a cloud whose every point is non-finite give *n_out = 0 and SVO_OK (point_voxel, when
 * given, is all -1).  The sums are serial by definition: a cloud that falls into one cell costs one dependent double addition per
 * point.  Left out: averaged normals (svo_cloud_estimate_normals runs after the down-sample, as in the recipe), PCL's VoxelGrid
 * (float centroids, a leaf origin at multiples of the leaf) and a down-sample inside svo_map_*.
 *
 * svo_voxel_grid: host code, no context -- steps 2 and 4 for a cloud's finite bounds: min_bound3 and the cells each axis spans
 * (INT64_MAX where the count passes 2^62).  SVO_OK; SVO_ERR_CAPACITY with both outputs written when an axis spans 2^21 cells or
 * more (what svo_voxel_downsample refuses); SVO_ERR_ARG with nothing written for a null pointer, a voxel_size as above, a bound
 * that is not finite or max below min.                                                                                          */
int svo_voxel_downsample(svo_ctx *ctx, const float *xyz, const float *color, int n, double voxel_size,
                         float *xyz_out, float *color_out, int *n_out, int *point_voxel, int *voxel_count, int mem);
int svo_voxel_grid(const float *min_xyz, const float *max_xyz, double voxel_size, double *min_bound3, int64_t *cells3);

/* ---- stereo rectification and undistortion: cv::stereoRectify -> initUndistortRectifyMap -> remap on both images of every
 * frame, and cv::undistortPoints -- what a raw rig (EuRoC MAV: radial-tangential distortion, a rotation between the cameras)
 * needs in front of every other entry point.  DESIGN.md section 10p; every recalled point and every choice of ours is numbered
 * in tests/rectify_numpy.py (N1 - N15).  Matrices are row-major doubles.
 *
 * The camera model: K (3 x 3), D with nD = 0, 4, 5 or 8 coefficients k1 k2 p1 p2 [k3 [k4 k5 k6]] (missing ones zero; D may be
 * NULL when nD is 0).  Thin-prism and tilt terms (12, 14) are refused.  All arithmetic is double, in the order of N2.
 *
 * svo_stereo_rectify: host only, no context -- Bouguet's algorithm with flags = 0 or SVO_CALIB_ZERO_DISPARITY and alpha = -1.
 * R, T: x2 = R x1 + T.  new_w x new_h: 0 x 0 or a size; with alpha = -1 it changes nothing (N7).  SVO_ERR_ARG, with nothing
 * written: a null pointer, an nD outside {0, 4, 5, 8}, a size that is not positive, alpha != -1 (the free scaling parameter and
 * the valid ROIs are not built), T = 0, an entry that is not finite.
 *
 * svo_rectify_map_create: the map of initUndistortRectifyMap(K, D, R, P, (w, h)) in OpenCV's fixed-point form -- per pixel an
 * int16 pair (the top-left tap) and a uint16 fraction word fy * 32 + fx in 1/32 steps -- built by one kernel and kept on the
 * device for the life of the handle.  R9 NULL = identity, P12 NULL = K.  src_w x src_h: the size of the images the map will
 * sample, which may differ from w x h.  Coordinates saturate to int16 (N12).
 * svo_rectify_map_from_float: the same words from a caller's own float maps (h x w each), converted as cv::remap converts them.
 * svo_rectify_map_get: xy [h][w][2] int16 and frac [h][w] uint16, where `mem` says.
 * svo_rectify_map_destroy: waits for the context's stream first; a NULL map is fine.
 *
 * svo_remap_batch: cv::remap(src, dst, map, INTER_LINEAR, BORDER_CONSTANT, border_value) on n_images (1..16) uint8 images of
 * src_h x src_w x c (c = 1, or 3 interleaved), back to back where `mem` says, as svo_sgbm_compute takes them -> n_images images
 * of h x w x c.  Weights 32 (32-a)(32-b) ... at 2^15, dst = (sum + 2^14) >> 15; a tap outside the source reads border_value
 * (0..255, the same byte for every channel).  One launch.  In device mode dst must not overlap src, and neither needs any
 * alignment.
 * svo_rectify_pairs: both maps (one size, one source size) over n_pairs (1..16) left and right images in ONE launch; bit for
 * bit what two svo_remap_batch calls give.
 *
 * svo_undistort_points: cv::undistortPoints(xy, K, D, R, P) on n float points: five fixed iterations, then R (NULL = none),
 * then P's fx, fy, cx, cy (NULL = normalised coordinates out); double inside, float out.  n = 0 is SVO_OK.  At most 2^24 points.
 * svo_undistort_points_host: the same arithmetic on the host with DOUBLE output and no context.
 *
 * Refusals: SVO_ERR_ARG with the outputs untouched (a null pointer, a count outside its range, c not 1 or 3, an unknown mem, a
 * singular P R, two maps of different sizes); SVO_ERR_CAPACITY for a w, h, src_w or src_h above 32767 (the int16 map) and for
 * more than 2^30 map pixels or source pixels per call.  Left out: alpha >= 0, fisheye, other interpolations and border modes,
 * 16-bit images.                                                                                                              */
typedef struct svo_rectify_map svo_rectify_map;
#define SVO_CALIB_ZERO_DISPARITY 1024
int svo_stereo_rectify(const double *K1, const double *D1, int nD1, const double *K2, const double *D2, int nD2, int w, int h,
                       const double *R, const double *T, int flags, double alpha, int new_w, int new_h, double *R1, double *R2,
                       double *P1, double *P2, double *Q);
int svo_rectify_map_create(svo_ctx *ctx, const double *K9, const double *D, int nD, const double *R9, const double *P12, int w,
                           int h, int src_w, int src_h, svo_rectify_map **map);
int svo_rectify_map_from_float(svo_ctx *ctx, const float *mapx, const float *mapy, int w, int h, int src_w, int src_h, int mem,
                               svo_rectify_map **map);
int svo_rectify_map_destroy(svo_ctx *ctx, svo_rectify_map *map);
int svo_rectify_map_get(svo_ctx *ctx, const svo_rectify_map *map, int16_t *xy, uint16_t *frac, int mem);
int svo_remap_batch(svo_ctx *ctx, const svo_rectify_map *map, const uint8_t *src, int n_images, int c, int border_value,
                    uint8_t *dst, int mem);
int svo_rectify_pairs(svo_ctx *ctx, const svo_rectify_map *map_left, const svo_rectify_map *map_right, const uint8_t *lefts,
                      const uint8_t *rights, int n_pairs, int c, int border_value, uint8_t *out_left, uint8_t *out_right, int mem);
int svo_undistort_points(svo_ctx *ctx, const float *xy, int n, const double *K9, const double *D, int nD, const double *R9,
                         const double *P12, float *out_xy, int mem);
int svo_undistort_points_host(const float *xy, int n, const double *K9, const double *D, int nD, const double *R9,
                              const double *P12, double *out_xy);

/* ---- dense stereo: StereoProcess::stereoMatch / reprojectDisparity, src/StereoCV.cpp:21-59,227-250 -- */
/* cv::StereoSGBM::create(1, 96, 7, 24, 96, 0, 60, 0, 3000, 5) + compute(grey1, grey2, disp) of
 * src/StereoCV.cpp:40-53 (MODE_SGBM: five paths, BT costs, median 3, filterSpeckles).  The recipe
 * and every recalled point of it: tests/sgbm_numpy.py, DESIGN.md section 10.                    */
enum { SVO_SGBM_MODE_SGBM = 0 };
typedef struct svo_sgbm_params {
    int min_disparity, num_disparities, block_size, p1, p2, disp12_max_diff,
        pre_filter_cap, uniqueness_ratio, speckle_window_size, speckle_range, mode;
} svo_sgbm_params;
/* the reference's values, src/StereoCV.cpp:40-51                                                 */
void svo_sgbm_default_params(svo_sgbm_params *p);
/* n_pairs (1..16) pairs of h x w x c images (c = 1 grey, c = 3 BGR converted as cvtColor BGR2GRAY,
 * src/StereoCV.cpp:37-38), back to back where `mem` says; disp: n_pairs x h x w int16, disparity
 * x 16, invalid = (min_disparity - 1) * 16.  SVO_ERR_ARG: num_disparities not a positive multiple
 * of 16 up to 256, an even block_size or one outside 1..11, p2 <= p1, w <= num_disparities +
 * min_disparity, an unknown mode.  SVO_ERR_CAPACITY: w > 2048 or more than 2^30 cost cells
 * (n_pairs x h x band columns x num_disparities) per call.                                       */
int svo_sgbm_compute(svo_ctx *ctx, const svo_sgbm_params *p, const uint8_t *left, const uint8_t *right,
                     int w, int h, int c, int n_pairs, int16_t *disp, int mem);
/* Q of cv::stereoRectify(K, 0, K, 0, size, I, (tx, 0, 0)) as src/StereoCV.cpp:229-234 calls it
 * (CALIB_ZERO_DISPARITY); Q16 row-major.  tx = +baseline is the reference's call (Q[3][2] < 0:
 * negative depths); tx = -baseline the conventional one.  Host only.       */
int svo_stereo_rectify_q(double fx, double fy, double cx, double cy, double tx, int w, int h, double *Q16);
/* disp.convertTo(CV_32F, disp_scale) + reprojectImageTo3D(disp, img3d, Q) + the loop of
 * src/StereoCV.cpp:240-249: pixels with Z > z_max or Z <= z_min skipped, (X, flip_y ? -Y : Y, Z)
 * and the image's B, G, R (grey replicated) as floats, row-major.  disp_scale 1 = the reference
 * (16 x the disparity), 1/16 = metric.  Q16: host.  xyz_out / bgr_out: w*h x 3 capacity (bgr_out
 * may be NULL, then image may be too).  *n_out is a HOST int in both modes.                     */
int svo_stereo_reproject(svo_ctx *ctx, const int16_t *disp, const uint8_t *image, int w, int h, int c,
                         const double *Q16, float disp_scale, float z_min, float z_max, int flip_y,
                         float *xyz_out, float *bgr_out, int *n_out, int mem);

/* ---- the disparity WLS filter around the matcher, src/StereoCV.cpp:25-28,51-59 (commented out upstream) ----
 * ximgproc::createDisparityWLSFilter(matcher) + createRightMatcher(matcher) + filter(disp, grey, out, rdisp): left-right
 * confidence from the two matchers' maps and their local variance, then the fast global smoother (three iterations of a
 * horizontal and a vertical tridiagonal solve per line) of disparity x confidence and of confidence, guided by the left
 * image.  The recipe, point by point (W1..W6, each marked recalled or ours): tests/wls_numpy.py, DESIGN.md section 10h;
 * the float32 operation order is fixed there and the results are bit-identical to that restatement.                    */
typedef struct svo_wls_params {
    double lambda, sigma_color;
    int lrc_thresh, depth_discontinuity_radius;
    float roll_off;
    int use_confidence;
    int roi_left, roi_right, roi_top, roi_bottom; /* offsets of the ROI from the image's four edges */
} svo_wls_params;
/* createDisparityWLSFilter(matcher)'s values for a left matcher (W2): lambda 8000, sigma 1.5, LRC threshold 24,
 * roll-off 0.001, radius ceil(block / 2), the ROI offsets from the matcher's disparity range and block.  The reference
 * then sets lambda 400 and sigma 0.4 (src/StereoCV.cpp:57-58).                                                       */
void svo_wls_default_params(const svo_sgbm_params *left, svo_wls_params *out);
/* createRightMatcher(matcher), SGBM case (W1); run it as svo_sgbm_compute(ctx, right_params, RIGHT, LEFT, ...)       */
void svo_sgbm_right_matcher_params(const svo_sgbm_params *left, svo_sgbm_params *right);
/* n_pairs (1..16) maps of h x w int16 (disparity x 16) from the left and the right matcher, guide: n_pairs x h x w x c
 * (c = 1 or 3) -> filtered: n_pairs x h x w int16 (the input left map outside the ROI), confidence (may be NULL):
 * n_pairs x h x w float, conf x 255, zero outside the ROI and all zero without use_confidence.  disp_right may be NULL
 * only when use_confidence == 0.  SVO_ERR_ARG, with the outputs untouched: n_pairs outside 1..16, c not 1 or 3, an
 * empty ROI or a negative offset, lambda < 0, sigma_color <= 0, depth_discontinuity_radius < 0.  SVO_ERR_CAPACITY: a
 * radius above 255, 2^30 pixels or more per call.                                                                    */
int svo_wls_filter(svo_ctx *ctx, const svo_wls_params *p, const int16_t *disp_left, const int16_t *disp_right,
                   const uint8_t *guide, int w, int h, int c, int n_pairs, int16_t *filtered, float *confidence, int mem);
/* The whole chain on the device: both matchers on the pairs (arguments as svo_sgbm_compute's; the right matcher only
 * when use_confidence is set or disp_right is asked for), grey conversion, the filter with the grey left image as guide.
 * disp_left, disp_right and confidence may be NULL.  Refusals are those of svo_sgbm_compute and svo_wls_filter, with
 * every output untouched.                                                                                             */
int svo_sgbm_wls_compute(svo_ctx *ctx, const svo_sgbm_params *sgbm, const svo_wls_params *wls, const uint8_t *left,
                         const uint8_t *right, int w, int h, int c, int n_pairs, int16_t *filtered, int16_t *disp_left,
                         int16_t *disp_right, float *confidence, int mem);

/* ---- block matching: cv::StereoBM, the dense matcher for frame rate ----
 * StereoBM::create(0, 21) + compute(left, right, disp): XSOBEL pre-filter, a block_size x block_size sum of absolute
 * differences per pixel and disparity, texture and uniqueness tests, sub-pixel winner, then validateDisparity
 * (disp12_max_diff >= 0) and filterSpeckles (speckle_window_size > 0, speckle_range >= 0); no median.  The output has
 * svo_sgbm_compute's format, so svo_stereo_reproject and svo_wls_filter take it as it is.  The recipe, point by point
 * (B1..B11, each marked recalled or ours): tests/bm_numpy.py; all integer, and the results are
 * bit-identical to that restatement.  Not built: PREFILTER_NORMALIZED_RESPONSE, roi1 / roi2, CV_32F output.             */
enum { SVO_BM_PREFILTER_NORMALIZED_RESPONSE = 0, SVO_BM_PREFILTER_XSOBEL = 1 };
typedef struct svo_bm_params {
    int pre_filter_type, pre_filter_size, pre_filter_cap, block_size, min_disparity, num_disparities,
        texture_threshold, uniqueness_ratio, speckle_window_size, speckle_range, disp12_max_diff;
} svo_bm_params;
/* StereoBM::create(0, 21)'s values (B1): XSOBEL, 9, 31, 21, 0, 64, 10, 15, 0, 0, -1                                     */
void svo_bm_default_params(svo_bm_params *p);
/* Arguments and output as svo_sgbm_compute's (invalid = (min_disparity - 1) * 16).  SVO_ERR_ARG, with the output
 * untouched: n_pairs outside 1..16, c not 1 or 3, num_disparities not a positive multiple of 16 up to 256, an even
 * block_size or one outside 5..255 or above min(w, h), pre_filter_cap outside 1..63, an even pre_filter_size or one
 * outside 5..255 (carried and checked; XSOBEL does not use it), a pre-filter type other than XSOBEL, a negative
 * texture_threshold or uniqueness_ratio, |min_disparity| above 2^20.  SVO_ERR_CAPACITY: block_size above 31, w > 2048,
 * 2^30 or more pixel x disparity cells (n_pairs x h x w x num_disparities) per call.  A disparity range that leaves no
 * band (B3) is no error: every pixel is invalid.                                                                       */
int svo_bm_compute(svo_ctx *ctx, const svo_bm_params *p, const uint8_t *left, const uint8_t *right,
                   int w, int h, int c, int n_pairs, int16_t *disp, int mem);
/* createRightMatcher(matcher), BM case (B11); run it as svo_bm_compute(ctx, right_params, RIGHT, LEFT, ...)             */
void svo_bm_right_matcher_params(const svo_bm_params *left, svo_bm_params *right);
/* createDisparityWLSFilter(matcher), BM case (B11): svo_wls_default_params' values with the radius ceil(0.33 * block)   */
void svo_wls_default_params_bm(const svo_bm_params *left, svo_wls_params *out);
/* svo_sgbm_wls_compute with the block matcher in the SGBM matcher's place (one body serves both).  Refusals are those of
 * svo_bm_compute and svo_wls_filter, with every output untouched.                                                       */
int svo_bm_wls_compute(svo_ctx *ctx, const svo_bm_params *bm, const svo_wls_params *wls, const uint8_t *left,
                       const uint8_t *right, int w, int h, int c, int n_pairs, int16_t *filtered, int16_t *disp_left,
                       int16_t *disp_right, float *confidence, int mem);
/* stage access for tests: the XSOBEL pre-filter (B2) of one h x w x c image (c = 3: grey first) with ftzero = cap -> out:
 * h x w bytes.  SVO_ERR_ARG: c not 1 or 3, cap outside 1..63, w or h below 1; SVO_ERR_CAPACITY: w > 2048 or 2^30 pixels.  */
int svo_bm_prefilter(svo_ctx *ctx, const uint8_t *image, int w, int h, int c, int cap, uint8_t *out, int mem);

/* ---- SIFT: detection and descriptors of OpenCV 3.2's xfeatures2d::SIFT (src/StereoCV.cpp:64-88, 123-147) ----
 * The reference pairs features by SIFT::create(N) -> detect / compute -> convertTo(CV_32F) -> BFMatcher().knnMatch(2) -> ratio
 * 0.8 -> findFundamentalMat; svo_sift_extract_batch produces the features, svo_knn_match (SVO_MATCH_L2_F32, dim 128) and
 * svo_ratio_pairs consume them.  The algorithm is the one tests/sift_numpy.py states operation by operation (DESIGN.md section
 * 10d): doubled first octave, nOctaves = cvRound(log2(min(2w, 2h)) - 2) + 1, n_octave_layers + 3 Gaussian layers per octave,
 * 26-neighbour extrema with the 5-step sub-pixel refinement, contrast and edge tests, 36-bin orientation histogram with peaks at
 * 0.8 of the maximum, the 4 x 4 x 8 descriptor clipped at 0.2 and stored as saturated bytes in floats (what convertTo(CV_32F)
 * yields).  Transcendentals are svo_exp / svo_cos / svo_sin of svo_math.h and OpenCV's fastAtan2 polynomial; histogram sums are
 * exact integer sums, so the result does not depend on the order lanes add in.
 *
 * Output: key points in ascending (octave, layer, row, column) order of the refined extremum, the orientations of one extremum in
 * ascending histogram bin; extrema whose refinement ends in the same cell are one key point (upstream's removeDuplicated).
 * n_features > 0 keeps every key point whose response is at or above the n_features-th largest, ties included (retainBest), so
 * an image can return more than n_features.  xy, size: full-resolution pixels (KeyPoint::pt, KeyPoint::size); angle: degrees in
 * [0, 360); response: |contrast|; octave: cv's packed field (octave in the low byte, -1 = 255 for the doubled frame; layer in the
 * second byte; the sub-layer offset in the third); desc: 128 floats per key point, integers 0 ... 255.
 *
 * svo_sift_extract_batch: n_images (1 ... 16) images of one size, w x h x c bytes each (c = 1, or 3 = BGR, converted with
 * cvtColor's integer weights); every output array holds n_images x cap entries, image i's at i * cap, n[i] of them valid; desc may
 * be NULL (detect only).  images: a host array of host or device pointers according to mem; n: HOST ints in both modes -- the
 * call waits once, for the counts.  SVO_ERR_ARG: null or misaligned (4 bytes) pointers, c not 1 or 3, n_octave_layers outside
 * 1 ... 8, w or h below 2 (the recipe's octave count would be 0) or above 16384, sigma <= 0 or so large that a Gaussian kernel
 * exceeds 255 taps, cap < 1, n_images outside 1 ... 16.  SVO_ERR_CAPACITY, two cases: (a) an image yields more than cap key points after
 * the filters -- every n[i] holds the needed count and the first min(n[i], cap) key points of each image are valid; (b) an image has
 * more than 65536 refined extrema or 131072 oriented key points before the filters (the work arrays) -- the call returns at that
 * image: the output arrays are left untouched (host memory) or unspecified (device memory), and n[] is written only up to and
 * including that image.  svo_last_error tells the two apart.  There is no CPU fallback.
 *
 * svo_sift_describe: detector->compute(image, keypoints, desc) for key points that came from elsewhere: the pyramid of `image` is
 * built as above and each key point is described in the layer its octave field names (scale and angle from size and angle).  A
 * key point whose octave field names no layer of this pyramid gets a zero descriptor.  On the key points svo_sift_extract_batch
 * returned it gives the same descriptors.  Every call builds the whole scale space again (it keeps nothing from an earlier
 * svo_sift_extract_batch on the same image): to describe the key points it detects, pass desc to svo_sift_extract_batch.
 *
 * svo_sift_pyramid (diagnostics: the parity tests compare every layer with the restatement): the Gaussian and DoG stacks of one
 * image, octave after octave, (n_octave_layers + 3) / (n_octave_layers + 2) planes of oh[o] x ow[o] floats each;
 * svo_sift_pyramid_layout gives the octave count and sizes (ow, oh: 16 ints each, or NULL).                              */
typedef struct svo_sift_params {
    int n_features;            /* 0 = all (cv: 0); the reference: 10000 / 20000 */
    int n_octave_layers;       /* 3 */
    double contrast_threshold; /* 0.04 */
    double edge_threshold;     /* 10 */
    double sigma;              /* 1.6 */
} svo_sift_params;
void svo_sift_default_params(svo_sift_params *p);
int svo_sift_extract_batch(svo_ctx *ctx, const uint8_t *const *images, int n_images, int w, int h, int c,
                           const svo_sift_params *prm, int cap, float *xy, float *size, float *angle, float *response, int *octave,
                           float *desc, int *n, int mem);
int svo_sift_describe(svo_ctx *ctx, const uint8_t *image, int w, int h, int c, const svo_sift_params *prm, const float *xy,
                      const float *size, const float *angle, const int *octave, int n, float *desc, int mem);
int svo_sift_pyramid_layout(int w, int h, int n_octave_layers, int *n_octaves, int *ow, int *oh);
int svo_sift_pyramid(svo_ctx *ctx, const uint8_t *image, int w, int h, int c, const svo_sift_params *prm, float *gauss, float *dog,
                     int mem);

/* ---- BRIEF: OpenCV 3.2's xfeatures2d::BriefDescriptorExtractor (src/StereoCV.cpp:66-75) -------------------------------
 * StereoProcess::stereoTriangulate describes its SIFT key points with BriefDescriptorExtractor::create() -> compute, converts the
 * bytes to floats and matches them with BFMatcher (L2): svo_sift_extract_batch (desc = NULL) finds the key points,
 * svo_brief_describe_batch describes them, svo_knn_match (SVO_MATCH_L2_U8, dim = bytes) and svo_ratio_pairs pair them.  The
 * algorithm is the one tests/brief_numpy.py states: grey by cvtColor's integer weights, the int32
 * integral image ((h + 1) x (w + 1), zero first row and column), KeyPointsFilter::runByImageBorder(28) -- a key point stays when
 * 28 <= cvRound(x) < w - 28 and the same for y, round half to even; an image with w <= 56 or h <= 56 keeps none --, and for test
 * t with the table row (y1, x1, y2, x2) the bit S(y1, x1) < S(y2, x2) at bit 7 - t % 8 of byte t / 8, S the 9 x 9 box sum
 * around ((int)(pt.y + 0.5) + y, (int)(pt.x + 0.5) + x).  One departure: a key point with (int)(x + 0.5) > w - 29 or
 * (int)(y + 0.5) > h - 29 -- only a half-integer coordinate on the far border -- is removed as well; upstream reads one column
 * or row past its integral image there.  use_orientation is not provided.
 *
 * The test table: upstream's generated_16/32/64.i are not part of this library.  The default tables are the library's own (both
 * end points Gaussian with sigma 48 / 5, clamped to +-24, tools/gen_brief_pattern.py): descriptors are format-compatible with
 * OpenCV's, not equal to them.  svo_brief_default_pattern copies the default of a descriptor length out (host only, no context):
 * 8 * bytes rows of (y1, x1, y2, x2).  svo_brief_set_pattern replaces the table of one length for this context (a host that has
 * OpenCV's tables sets them here); NULL brings the default back.  SVO_ERR_ARG: an entry outside +-24, a test with equal end points.
 *
 * svo_brief_describe_batch: n_images (1 ... 16) images of one size, w x h x c bytes each (c = 1, or 3 = BGR); images: a host array
 * of host or device pointers according to mem.  Image i's key points are the n_in[i] <= cap (x, y) pairs at xy + 2 * i * cap
 * (xy follows mem; n_in: HOST ints in both modes).  Outputs at row i * cap (they follow mem): desc, `bytes` (16, 32 or 64) per kept
 * key point, and kept_index, the index of each kept key point among the image's n_in[i], ascending -- the order is preserved.
 * n_out[i], HOST ints in both modes, is the number kept: the call waits once, for the counts.  In device mode the outputs must not
 * overlap xy.  SVO_ERR_ARG: null or misaligned (4 bytes: xy, n_in, kept_index, n_out) pointers, c not 1 or 3, bytes not 16 / 32 /
 * 64, n_images outside 1 ... 16, cap < 1, an n_in[i] outside 0 ... cap, w or h below 1 or above 16384.  SVO_ERR_CAPACITY:
 * 255 w h > 2^31 - 1 (the int32 integral image could overflow), decided before anything is allocated.  Nothing is written when a
 * call is refused.  A batch returns the same bits as one call per image, host memory the same as device memory.
 *
 * svo_brief_integral (diagnostics: the parity tests read the table): the (h + 1) x (w + 1) int32 integral image of one image.   */
int svo_brief_default_pattern(int bytes, int8_t *pattern);
int svo_brief_set_pattern(svo_ctx *ctx, int bytes, const int8_t *pattern);
int svo_brief_describe_batch(svo_ctx *ctx, const uint8_t *const *images, int n_images, int w, int h, int c, int bytes,
                             const float *xy, const int *n_in, int cap, int *kept_index, uint8_t *desc, int *n_out, int mem);
int svo_brief_integral(svo_ctx *ctx, const uint8_t *image, int w, int h, int c, int32_t *sum, int mem);

/* ---- SURF: detection and descriptors of OpenCV 3.2's xfeatures2d::SURF (src/bundleAdjust.cpp:236-317, include/trangulation.h:32-61) ----
 * The older pipeline pairs features by SURF::create(500) -> detect / compute -> BFMatcher().knnMatch(2) -> ratio 0.8 ->
 * triangulatePoints; svo_surf_extract_batch produces the features, svo_knn_match (SVO_MATCH_L2_F32, dim 64) and svo_ratio_pairs
 * consume them.  The algorithm is the one tests/surf_numpy.py states operation by operation: the int32
 * integral image of the grey image, for octave o and layer l (0 ... n_octave_layers + 1) the box-filter Hessian of size
 * (9 + 6 l) << o sampled every 1 << o pixels (det = dxx dyy - 0.81 dxy^2, trace = dxx + dyy), maxima of the middle layers above the
 * threshold and their 26 neighbours, the 3 x 3 x 3 interpolation, the dominant orientation from 113 Haar samples in a 60 degree
 * window moved in steps of 5 degrees, the 64-float descriptor from the rotated window of (int)(21 s) pixels a side (s = size * 1.2
 * / 9) reduced to 21 x 21 by area averaging.  Transcendentals are svo_exp / svo_cos / svo_sin of svo_math.h and OpenCV's fastAtan2
 * polynomial; every float sum has a stated order, so the result does not depend on how lanes are scheduled.
 *
 * Output: key points in KeypointGreater's order (response descending, then size, octave, y descending, x ascending), remaining ties
 * by ascending (octave, layer, row, column) of the sample: a total order.  xy, size: pixels (KeyPoint::pt, KeyPoint::size); angle:
 * degrees in [0, 360) (270 with upright); response: the determinant; octave: 0 ... n_octaves - 1; laplacian: KeyPoint::class_id, the
 * sign of the trace (-1, 0, 1); desc: 64 floats per key point, unit norm.  A key point whose orientation wavelet does not fit the
 * image, or that has no orientation sample inside it, is dropped, as upstream drops it.
 *
 * svo_surf_extract_batch: n_images (1 ... 16) images of one size, w x h x c bytes each (c = 1, or 3 = BGR, converted with
 * cvtColor's integer weights); every output array holds n_images x cap entries, image i's at i * cap, n[i] of them valid; desc may
 * be NULL (detect only).  images: a host array of host or device pointers according to mem; n: HOST ints in both modes -- the
 * call waits once, for the counts.  SVO_ERR_ARG: null or misaligned (4 bytes) pointers, c not 1 or 3, n_octaves or n_octave_layers
 * outside 1 ... 8, a negative or non-finite hessian_threshold, extended != 0 (the 128-float descriptor is not provided), w or h
 * below 1 or above 16384, 255 w h > 2^31 - 1 (the int32 integral image could overflow), cap < 1, n_images outside 1 ... 16; nothing
 * is written then.  SVO_ERR_CAPACITY, two cases: (a) an image yields more than cap key points -- every n[i] holds the needed count
 * and the first min(n[i], cap) key points of each image are valid; (b) an image has more than 65536 key points (the work arrays)
 * -- the call returns at that image: the output arrays are left untouched (host memory) or unspecified (device memory), and n[] is
 * written only up to and including that image.  A batch returns the same bits as one call per image, host memory the same as
 * device memory.  There is no CPU fallback.
 *
 * svo_surf_describe: detector->compute(image, keypoints, desc) for n key points that came from elsewhere (xy, size): angle_out,
 * desc (64 floats each) and kept (1 / 0) per key point, in the input order.  A key point that upstream would drop (see above), one
 * whose position is not finite or beyond +-65536, or whose window (int)(21 s) is not in 21 ... 65536, has kept 0, angle -1 and a zero
 * descriptor.  On the key points svo_surf_extract_batch returned it gives the same angles and descriptors.
 *
 * svo_surf_layers (diagnostics: the parity tests compare every plane with the restatement): the det and trace planes of one image,
 * octave after octave, n_octave_layers + 2 planes of (h >> o) x (w >> o) floats each; svo_surf_layers_layout gives, per plane, the
 * filter size, the sample step and the plane's width and height (n_octaves * (n_octave_layers + 2) ints each, any may be NULL). */
typedef struct svo_surf_params {
    double hessian_threshold;  /* 100; the reference: 500 / 1200 */
    int n_octaves;             /* 4 */
    int n_octave_layers;       /* 3 */
    int extended;              /* 0; anything else is refused */
    int upright;               /* 0 */
} svo_surf_params;
void svo_surf_default_params(svo_surf_params *p);
int svo_surf_extract_batch(svo_ctx *ctx, const uint8_t *const *images, int n_images, int w, int h, int c,
                           const svo_surf_params *prm, int cap, float *xy, float *size, float *angle, float *response, int *octave,
                           int *laplacian, float *desc, int *n, int mem);
int svo_surf_describe(svo_ctx *ctx, const uint8_t *image, int w, int h, int c, const svo_surf_params *prm, const float *xy,
                      const float *size, int n, float *angle_out, float *desc, uint8_t *kept, int mem);
int svo_surf_layers(svo_ctx *ctx, const uint8_t *image, int w, int h, int c, const svo_surf_params *prm, float *det, float *trace,
                    int mem);
int svo_surf_layers_layout(int w, int h, int n_octaves, int n_octave_layers, int *sizes, int *steps, int *lw, int *lh);

/* ---- two-view monocular geometry: StereoProcess::monocularTriangulate, src/StereoCV.cpp:123-188 ---- */
/* OpenCV 3.2's five-point solver (EMEstimatorCallback::runKernel, Nister's method) on nsamples
 * independent 5-samples of NORMALISED double coordinates: x1n / x2n nsamples x 5 x 2, x2^T E x1 = 0.
 * E_out: nsamples x 10 x 9 (row-major 3x3 each, unit Frobenius norm, the entry of largest magnitude
 * positive, in ascending order of the solver's z root; unused slots zero); nsol: nsamples ints
 * (0..10).  Arrays follow `mem`.  The solver's choices: DESIGN.md section 10b.                 */
int svo_essential_5pt(svo_ctx *ctx, const double *x1n, const double *x2n, int nsamples, double *E_out, int *nsol,
                      int mem);
/* cv::findEssentialMat(p1, p2, K, RANSAC, confidence, threshold, mask) for nprob (1..16) problems:
 * problem k is pairs offsets[k] .. offsets[k+1]-1 of p1 / p2 (float x, y pixels) with
 * K4[4k .. 4k+3] = fx, fy, cx, cy.  offsets (nprob + 1 ints) and K4 are HOST memory always.  Points
 * are normalised by K in double; the Sampson error (float) is tested against
 * (threshold / ((fx + fy) / 2))^2; 5-samples are drawn like svo_pnp_ransac's, keyed by (seed,
 * iteration); first-best-wins with the adaptive bound, max_iters 1..20000 (OpenCV: 1000).  Below five
 * pairs: no model; exactly five: every solution of the solver, mask all ones, iters_run 0.  mask:
 * a byte per pair (1 = inlier).  Per problem (optional, following `mem`): E_out 10 x 9 doubles (the
 * winning model in slot 0; with five pairs, every solution), nmodels, inlier_count, iters_run.  A
 * batch gives the same bits as its problems one call at a time.                                    */
int svo_find_essential(svo_ctx *ctx, const float *p1, const float *p2, const int *offsets, int nprob, const double *K4,
                       double threshold, double confidence, int max_iters, uint64_t seed, uint8_t *mask,
                       double *E_out, int *nmodels, int *inlier_count, int *iters_run, int mem);
/* cv::recoverPose(E, p1, p2, K, R, t, distance_thresh, mask) for nprob (1..16) problems laid out as
 * svo_find_essential's; E9: nprob x 9.  The four decompositions of E are tested by triangulating
 * every pair (DLT, normalised coordinates, double): a pair counts when Q2 Q3 > 0, its depth in
 * camera 1 is below distance_thresh (OpenCV: 50) and its depth in camera 2 is in (0, distance_thresh);
 * a non-null mask_inout is ANDed in and receives the chosen candidate's mask.  The first candidate
 * with the largest count wins (OpenCV's order).  R9 (nprob x 9), t3 (nprob x 3, unit norm), good
 * (optional, nprob ints) follow `mem` like the point arrays; offsets / K4 are host memory.         */
int svo_recover_pose(svo_ctx *ctx, const double *E9, const float *p1, const float *p2, const int *offsets, int nprob,
                     const double *K4, double distance_thresh, uint8_t *mask_inout, double *R9, double *t3, int *good,
                     int mem);
/* cv::decomposeEssentialMat: R1 = U W V^T, R2 = U W^T V^T, t = u3 (W = [[0,1,0],[-1,0,0],[0,0,1]]).
 * The SVD's signs are fixed so that each of the first two right singular vectors has its entry of
 * largest magnitude positive, and u3 = u1 x u2, v3 = v1 x v2 (det +1).  Host only.                 */
int svo_decompose_essential(const double *E9, double *R1, double *R2, double *t);

/* ---- planar two-view geometry: cv::findHomography (RANSAC), cv::decomposeHomographyMat and the pose they give ---- */
/* The minimal solver on nsamples independent 4-samples: x1 / x2 nsamples x 4 x 2 doubles, x2 ~ H x1.  checkSubset first
 * (no three of the four points collinear in either image, every triple turning the same way in both), then the 8 x 8
 * system with h8 = 1 in normalised coordinates.  H_out: nsamples x 9, row-major, h8 = 1; ok: nsamples ints, 0 for a
 * rejected or singular sample, whose slot is zero.  Arrays follow `mem`.  The solver's choices: DESIGN.md section 10r. */
int svo_homography_4pt(svo_ctx *ctx, const double *x1, const double *x2, int nsamples, double *H_out, int *ok, int mem);
/* cv::findHomography(p1, p2, RANSAC, threshold, mask, max_iters, confidence) for nprob (1..16) problems: problem k is
 * pairs offsets[k] .. offsets[k+1]-1 of p1 / p2 (float x, y pixels); offsets (nprob + 1 ints) are HOST memory always.
 * OpenCV's defaults: threshold 3.0, max_iters 2000 (here 1..20000), confidence 0.995.  4-samples are drawn like
 * svo_pnp_ransac's, keyed by (seed, iteration); a sample that checkSubset rejects is drawn again at most 8 times, after
 * which its iteration scores no model.  The float forward transfer error is tested against threshold^2; first-best-wins
 * with the adaptive bound.  The winner is refitted over its inliers (normalised DLT) and polished by at most ten
 * Levenberg-Marquardt steps on h0 .. h7 in double.  mask: a byte per pair (1 = inlier), the loop's, not recomputed after
 * the polish.  Per problem (optional, following `mem`): H_out 9 doubles (h8 = 1), inlier_count, iters_run.  Below four
 * pairs, or when every sample is rejected: count 0, mask zero, H_out zero.  Exactly four: the minimal solution, mask all
 * ones, iters_run 0.  A batch gives the same bits as its problems one call at a time.                                */
int svo_find_homography(svo_ctx *ctx, const float *p1, const float *p2, const int *offsets, int nprob, double threshold,
                        double confidence, int max_iters, uint64_t seed, uint8_t *mask, double *H_out, int *inlier_count,
                        int *iters_run, int mem);
/* cv::decomposeHomographyMat.  Hn = K^-1 H K (K4 = fx, fy, cx, cy) with det Hn > 0, scaled so that its middle singular
 * value is 1; then Hn = R + t n^T.  Up to four (R, t / d, n) with det R = +1 and |n| = 1 in the order (Ra, ta, na),
 * (Ra, -ta, -na), (Rb, tb, nb), (Rb, -tb, -nb): of (t, n) and (-t, -n) the first has nz > 0 (nz = 0: ny > 0, then
 * nx > 0); `a` is the solution whose first normal is the larger by (nz, ny, nx).  When the largest and smallest
 * eigenvalues of Hn^T Hn differ by at most 1e-8 (a pure rotation): one solution, t = 0, n = (0, 0, 1).  R: 4 x 9,
 * t, n: 4 x 3 (unused slots zero); *nsol: 0 (singular H), 1 or 4.  Host only.                                        */
int svo_decompose_homography(const double *H9, const double *K4, double *R, double *t, double *n, int *nsol);
/* The pose of a plane-induced homography for nprob (1..16) problems laid out as svo_find_homography's; H9: nprob x 9,
 * K4: nprob x 4 (host memory).  Each candidate of svo_decompose_homography is scored by svo_recover_pose's test:
 * every pair is triangulated with [R | t / |t|]; it counts when Q2 Q3 > 0, its depth in camera 1 is below
 * distance_thresh and its depth in camera 2 is in (0, distance_thresh); a non-null mask_inout is ANDed in and receives
 * the chosen candidate's mask.  The first candidate with the largest count wins.  R9 (nprob x 9), t3 (nprob x 3: unit
 * norm, or zero for the pure rotation), n3 (nprob x 3) and good4 (optional, nprob x 4: every candidate's count, so that a
 * tie between two candidates shows) follow `mem` like the point arrays.  A singular H gives zeros.                 */
int svo_homography_pose(svo_ctx *ctx, const double *H9, const float *p1, const float *p2, const int *offsets, int nprob,
                        const double *K4, double distance_thresh, uint8_t *mask_inout, double *R9, double *t3, double *n3,
                        int *good4, int mem);

/* ---- descriptor matching: cv::BFMatcher(normType, false).knnMatch + the ratio test ----------------------------------
 * The block the reference runs wherever it pairs features outside the dense grid (src/triangulation.cpp:120-133, the
 * DENSE_FLAG == false branch of stereoTriangulate; src/StereoCV.cpp:77-88,136-147; src/bundleAdjust.cpp:269-271):
 *   desc.convertTo(CV_32F); BFMatcher().knnMatch(desc1, desc2, matches, 2); keep m if m.distance < 0.8 * n.distance
 * svo_knn_match runs knnMatch for nprob (1..16) independent problems: problem p matches query rows q_offsets[p] ..
 * q_offsets[p+1]-1 against train rows t_offsets[p] .. t_offsets[p+1]-1 (offsets: nprob + 1 ints each, HOST memory
 * always).  Descriptors are row-major, `dim` elements per row, and are read as 32-bit words: both arrays 4-byte aligned.
 * idx / dist hold k entries per query row (row r of the query array at r * k), best first, and follow `mem`; train
 * indices are local to the problem.
 *   norm              elements      dim                  selection key                       dist
 *   SVO_MATCH_L2_F32  float         1..256               s (below)                           float sqrt(s)
 *   SVO_MATCH_L2_U8   bytes         4..256, multiple of 4  sum (a_i - b_i)^2 in integers     float sqrt of the exact integer
 *   SVO_MATCH_HAMMING uint32 words  1..16 (ORB: 8)       popcount of the xor                 the count as a float
 * The float key: s = 0; for i in 0..dim-1: t = a_i - b_i; s = s + t*t -- every operation a float operation of its own,
 * in index order, one accumulator, no FMA (direct differences: the |a|^2 + |b|^2 - 2ab expansion rounds differently and
 * loses the small distances the ratio test reads).  Both square roots are correctly rounded.  SVO_MATCH_L2_U8 is the
 * reference's live case -- ORB / BRIEF bytes cast to CV_32F: with dim <= 256 the sum stays below 2^24, every partial sum
 * is an exact float, so it returns the same bits as SVO_MATCH_L2_F32 on the converted floats in ANY summation order.
 * Order: ascending key, equal keys to the LOWER train index; selection is on the key, not on the rooted value; a NaN
 * key orders behind every number.  With fewer than k train rows the missing slots are idx -1, dist +inf; a problem
 * without queries writes nothing.  k: 1..4.  At most 32768 queries and 32768 train rows per problem
 * (SVO_ERR_CAPACITY).  SVO_ERR_ARG: an unknown norm, a bad dim or k, decreasing offsets, null or misaligned pointers.
 * A batch returns the same bits as its problems one call at a time.  No nq x nt distance matrix is formed in memory
 * (csrc/match.hip).                                                                             */
enum { SVO_MATCH_L2_F32 = 0, SVO_MATCH_L2_U8 = 1, SVO_MATCH_HAMMING = 2 };
int svo_knn_match(svo_ctx *ctx, int norm, const void *query, const void *train, int dim, const int *q_offsets,
                  const int *t_offsets, int nprob, int k, int *idx, float *dist, int mem);
/* The filter loop of src/triangulation.cpp:127-133 for ONE problem: query i (0 .. nq-1; idx / dist: nq x k as
 * svo_knn_match writes them) is kept when k >= 2, idx[i*k+1] >= 0 and (double)dist[i*k] < ratio * (double)dist[i*k+1]
 * -- the comparison in double, as the C++ expression performs it.  Kept pairs in query order: p1[j] = xy_query[i],
 * p2[j] = xy_train[idx[i*k]] (x, y floats; p1 / p2: nq pairs capacity).  mask (optional): a byte per query, 1 = kept.
 * *count is a HOST int in both modes (the call synchronises for it).  Device outputs must not overlap the inputs.
 * Every idx[i*k] must be -1 or name a valid xy_train row: the call has no train count to check it against (host mode
 * stages xy_train up to the largest idx[i*k]).
 * At most 32768 queries.                                                                                              */
int svo_ratio_pairs(svo_ctx *ctx, const int *idx, const float *dist, int nq, int k, double ratio, const float *xy_query,
                    const float *xy_train, float *p1, float *p2, uint8_t *mask, int *count, int mem);
/* ---- cross-check, radius and masked matching: the rest of cv::BFMatcher ---------------------------------------------
 * The three calls below share svo_knn_match's conventions: the norms and their selection keys, the order (ascending key,
 * equal keys to the lower index, a NaN key behind every number), batches of 1..16 problems over host offset arrays that
 * return the bits of their problems one call at a time, `mem`, 4-byte alignment, 32768 rows per problem
 * (SVO_ERR_CAPACITY), SVO_ERR_ARG; a refusal leaves every output untouched.  None forms an nq x nt matrix in memory.
 *
 * svo_match_cross: BFMatcher(norm, true).match.  idx / dist: ONE entry per query row; a query without a partner gets
 * -1 / +inf.  Every comparison is made on the selection key, never on the rooted float (ours: two keys whose roots round
 * to the same float still order by key).
 *   SVO_CROSS_MUTUAL  query i is paired with train j exactly when j is i's best train row and i is j's best query row,
 *                     both by the order above (a NaN key takes part like any other key: behind every number).
 *   SVO_CROSS_CV      what batchDistance(..., crosscheck = true) of OpenCV 3.2 does, as recalled: only the reverse search
 *                     runs -- each train row finds its best query, and a query keeps, among the train rows that chose it,
 *                     the one with the smallest key (strict < over ascending train rows: the lower train row wins a
 *                     tie).  A train row whose best key is NaN chooses nobody (d < d0 is false).  A query can be paired
 *                     here although its own best train row is another one: without NaN keys, CV keeps MUTUAL's pairs and adds to them.
 * The call queues the reverse search (the kernels of svo_knn_match with the roles swapped), for MUTUAL the forward
 * search, and one pairing kernel; in device mode it waits for nothing.                                                */
enum { SVO_CROSS_MUTUAL = 0, SVO_CROSS_CV = 1 };
int svo_match_cross(svo_ctx *ctx, int norm, const void *query, const void *train, int dim, const int *q_offsets,
                    const int *t_offsets, int nprob, int mode, int *idx, float *dist, int mem);
/* svo_radius_match: BFMatcher::radiusMatch -- for every query all train rows with dist <= max_distance, compared on the
 * float that is returned (rooted for the two L2 norms, the count for HAMMING); a NaN dist never passes, a negative
 * max_distance admits nothing, a NaN max_distance is SVO_ERR_ARG.  Each query's matches are in the order above.
 * Output is CSR: row_offsets has a block of nq_p + 1 ints per problem, problem p's at row_offsets[q_offsets[p] + p]
 * (q_offsets[nprob] + nprob ints in all); query i of problem p owns idx / dist [o[i], o[i + 1]), positions in the flat
 * arrays of `capacity` entries (a problem's first offset is the previous problem's last); train indices are local to
 * the problem.  row_offsets, idx and dist follow `mem`; *total is a HOST int, the call waits once for it (and once more
 * for the copies of a host call).  SVO_ERR_CAPACITY when the total exceeds `capacity` or one query has more than
 * SVO_RADIUS_MAX_PER_QUERY matches (one query's sort is held in LDS: 8192 entries of 8 bytes, two workgroups in a CU's
 * 160 KB): then row_offsets holds the offsets that would be needed (saturated at INT_MAX), *total their sum, and nothing
 * else is written.                                                                                                    */
#define SVO_RADIUS_MAX_PER_QUERY 8192
int svo_radius_match(svo_ctx *ctx, int norm, const void *query, const void *train, int dim, const int *q_offsets,
                     const int *t_offsets, int nprob, float max_distance, int *row_offsets, int *idx, float *dist,
                     int capacity, int *total, int mem);
/* svo_knn_match_gated: knnMatch with a mask -- svo_knn_match over the allowed (query, train) pairs only, in one of two
 * forms (exactly one must be given, the other's pointers null):
 *   mask      bytes, nonzero = allowed: problem p's nq_p x nt_p row-major matrix, the problems' matrices back to back
 *             (cv::BFMatcher's `mask` argument); follows `mem`.
 *   gate      no matrix exists: xy_query / xy_train (x, y floats per row of the query / train arrays, following `mem`)
 *             and *gate (host).  Train row t is a candidate of query q when |y_q - y_t| <= dy_max and
 *             dx_min <= x_q - x_t <= dx_max -- the subtraction, the absolute value and each comparison a float operation
 *             of its own, in that order; a NaN anywhere fails.  A rectified pair: dy_max = the row tolerance, dx_min 0,
 *             dx_max the largest disparity.
 * A query with fewer than k candidates gets -1 / +inf in the missing slots.  Where every pair is allowed the result is
 * svo_knn_match's, bit for bit.                                                                                        */
typedef struct svo_match_gate {
    float dy_max, dx_min, dx_max;
} svo_match_gate;
int svo_knn_match_gated(svo_ctx *ctx, int norm, const void *query, const void *train, int dim, const int *q_offsets,
                        const int *t_offsets, int nprob, int k, const uint8_t *mask, const float *xy_query,
                        const float *xy_train, const svo_match_gate *gate, int *idx, float *dist, int mem);

/* ---- loop-closure detection: features ---------------------------------------------------------- */
/* cv::ORB::create()->detectAndCompute(img, Mat(), kp, desc) of visualSLAM::checkLoopDetectorStatus,
 * src/optimizationStuff.cpp:49-56.  image: h x w x c (BGR or grey).  Up to n_features (500
 * upstream) oriented-FAST keypoints over 3 octaves with 256-bit steered binary descriptors (the
 * recipe and its stated differences from cv::ORB: oracle/orb.c).  Outputs, n_features
 * capacity: xy (level-0 pixels), octave, response, dir (unit orientation vector), desc (8 words
 * per keypoint); octave / response / dir may be NULL.  *n is a HOST int in both modes.            */
int svo_orb_extract(svo_ctx *ctx, const uint8_t *image, int w, int h, int c, int n_features, int fast_threshold,
                    float *xy, int *octave, float *response, float *dir, uint32_t *desc, int *n, int mem);

/* The same call in cv::ORB's OWN shape (round 5): ORB::create()'s defaults -- 8 levels of scale 1.2 built level from level by
 * cv::resize(INTER_LINEAR), upstream's per-level feature quota, FAST-9/16 with its score-based suppression, retainBest(2q) by
 * the FAST score, Harris ranking, retainBest(q), orientation through fastAtan2, tests on GaussianBlur(7x7, 2) -- so that a
 * DBoW2 vocabulary trained on cv::ORB descriptors (the reference's orb_voc00.yml.gz, include/visualSLAM.h:131-134) meets
 * descriptors of the shape it was trained on.  The recipe: oracle/orb.c:orc_orb_extract_cv.  shape 0 keeps the three
 * factor-2 octaves of svo_orb_extract.                                                                              */
enum { SVO_ORB_SHAPE_OCTAVES3 = 0, SVO_ORB_SHAPE_CV = 1 };
typedef struct svo_orb_params {
    int n_features;     /* 500 */
    int fast_threshold; /* 20 */
    int shape;          /* SVO_ORB_SHAPE_CV */
    int n_levels;       /* 8 (shape CV only; at most 8) */
    float scale_factor; /* 1.2f */
} svo_orb_params;
void svo_orb_default_params(svo_orb_params *p);
/* The 256 x 4 sampling pattern of the binary tests (x1 y1 x2 y2 per test, |coordinate| <= 15): cv::ORB's learned
 * bit_pattern_31_ lives in the OpenCV sources, which the reference does not vendor -- a host that has them sets it here
 * (pattern[i] = bit_pattern_31_[i]); NULL restores the seeded default of oracle/orb.c.  Applies to shape CV on this context
 * (svo_orb_extract_batch, and detectors created on the context AFTER the call).                                     */
int svo_orb_set_pattern(svo_ctx *ctx, const int8_t *pattern_256x4);
/* n_images images of one size in ONE set of launches (blockIdx.z = image; groups of 32).  images: host array of n_images
 * pointers to images that live where `mem` says.  Outputs hold n_images x n_features entries (image i at i * n_features),
 * where `mem` says; octave / response / dir may be NULL; dir = (cos, sin) of the key point's angle.  n: HOST ints, one per
 * image.  prm NULL = the defaults.                                                                                    */
int svo_orb_extract_batch(svo_ctx *ctx, const uint8_t *const *images, int n_images, int w, int h, int c, const svo_orb_params *prm,
                          float *xy, int *octave, float *response, float *dir, uint32_t *desc, int *n, int mem);

/* ---- loop-closure detection: visualSLAM::checkLoopDetectorStatus, src/optimizationStuff.cpp:49-64 */
/* = cv::ORB features + DLoopDetector::detectLoop (include/TemplatedLoopDetector.h:696-861).  The
 * detector keeps every frame's features in HBM; one svo_lc_detect call per frame, in order.
 * Defaults: Parameters::set(1) (:552-568) overridden as visualSLAM does (include/visualSLAM.h:
 * 120-127: use_nss, alpha 0.9, k 1).  The bag-of-words score is replaced by a vocabulary-free
 * descriptor-matching similarity (the vocabulary was stripped from the reference).     */
typedef struct svo_lc svo_lc;
typedef struct svo_lc_params {
    int n_features;               /* 500                                                          */
    int fast_threshold;           /* 20                                                           */
    int hamming_threshold;        /* 64: a query descriptor "finds" an entry within this radius   */
    int max_entries;              /* database capacity in frames (8192; with a vocabulary at most 16384) */
    int use_nss;                  /* 1                                                            */
    float alpha;                  /* 0.9                                                          */
    int k;                        /* 1: more than k temporally consistent matches                 */
    int dislocal;                 /* 20                                                           */
    int max_db_results;           /* 50                                                           */
    float min_nss_factor;         /* 0.005                                                        */
    int min_matches_per_group, max_intragroup_gap, max_distance_between_groups,
        max_distance_between_queries;                                   /* 1, 3, 3, 2             */
    int min_Fpoints, max_ransac_iterations;                              /* 12, 500               */
    double ransac_probability, max_reprojection_error, max_neighbor_ratio; /* 0.99, 2.0, 0.6      */
    uint64_t seed;                /* RANSAC sampling seed of the geometric check                  */
    int orb_shape;                /* SVO_ORB_SHAPE_CV (1): cv::ORB's own pyramid and pipeline; 0: three factor-2 octaves */
    int orb_levels;               /* 8   */
    float orb_scale_factor;       /* 1.2 */
} svo_lc_params;
enum { /* DLoopDetector::DetectionStatus, include/TemplatedLoopDetector.h:51-69 */
    SVO_LC_LOOP_DETECTED = 0,
    SVO_LC_CLOSE_MATCHES_ONLY = 1,
    SVO_LC_NO_DB_RESULTS = 2,
    SVO_LC_LOW_NSS_FACTOR = 3,
    SVO_LC_LOW_SCORES = 4,
    SVO_LC_NO_GROUPS = 5,
    SVO_LC_NO_TEMPORAL_CONSISTENCY = 6,
    SVO_LC_NO_GEOMETRICAL_CONSISTENCY = 7
};
void svo_lc_default_params(svo_lc_params *p);
/* SVO_ERR_ARG, with *out NULL: n_features outside 8..2048, max_entries < 2, dislocal < 0, k < 0, alpha outside 0..1 (or not a
 * number), max_db_results outside 1..64.                                                                             */
int svo_lc_create(svo_ctx *ctx, const svo_lc_params *params, int width, int height, int channels, svo_lc **out);
int svo_lc_destroy(svo_lc *lc);
int svo_lc_size(const svo_lc *lc);
/* detectLoop for the next frame: *status = DetectionStatus, *query = this frame's entry id,
 * *match = the matched entry (-1 if none); a detection is status == SVO_LC_LOOP_DETECTED.        */
int svo_lc_detect(svo_lc *lc, const uint8_t *image, int mem, int *status, int *query, int *match);
/* The same in two halves, so that the detector never holds up the frame loop (src/VisualSLAM.cpp:54-169 calls
 * checkLoopDetectorStatus inside it): svo_lc_submit queues the frame's features, its scoring against the database
 * and a reduction of the scores to the <= max_db_results candidates the host logic reads (one small record in
 * pinned memory) on the detector's OWN context and returns at once; svo_lc_collect gives the verdict of the oldest
 * queued frame (it waits, on the detector's streams only, if that frame is not through yet).  Frames are collected in
 * the order they were submitted; svo_lc_pending = queued and not collected.  Give the detector a context of its
 * own (svo_ctx_create) and it runs beside the front-end's streams.  A collect forms the verdicts of every queued frame
 * whose record has landed (up to 16) and runs the geometric checks they need -- matching, pair lists and the F-matrix
 * RANSACs, all on the device -- as one chain of launches on a second stream the detector owns, behind the event of their
 * group of frames; it waits for that chain only, and has started the following group's before it does. */
int svo_lc_submit(svo_lc *lc, const uint8_t *image, int mem);
int svo_lc_collect(svo_lc *lc, int *status, int *query, int *match);
/* The verdicts of the n oldest queued frames in one call (n svo_lc_collect calls; n <= svo_lc_pending): arrays of n. */
int svo_lc_collect_batch(svo_lc *lc, int n, int *status, int *query, int *match);
/* n frames at once (round 5): with orb_shape CV and a vocabulary the features of up to 16 images come out of ONE set of
 * launches and so does every stage of their scoring (16 <= dislocal: no frame of a group can be another's candidate); the
 * verdicts -- collected one by one with svo_lc_collect as ever -- are those of n svo_lc_submit calls, bit for bit.
 * images: host array of n pointers; device images must stay valid until the last frame has been collected.          */
int svo_lc_submit_batch(svo_lc *lc, const uint8_t *const *images, int n, int mem);
int svo_lc_pending(const svo_lc *lc);

/* ---- the vocabulary: OrbVocabulary of DBoW2 (include/visualSLAM.h:115-137 loads orb_voc00.yml.gz; the reference's own
 * trainer: src/bagOfWordsDetector.cpp:46-56, OrbVocabulary(k = 9, L = 6, TF_IDF, L1_NORM).create(features)) ------------
 * A tree of 256-bit centres: node 0 is the root, the children of a node have consecutive ids, the leaves are the words
 * (numbered in node order), every word carries its idf weight.  svo_voc_create takes the arrays of a vocabulary that was
 * loaded from a file (ros_stereo_slam_amd/vocabulary.py reads DBoW2's .yml / .yml.gz); svo_voc_train builds one on the GPU
 * by hierarchical k-medians++ in Hamming space from host descriptors (8 words each; image i owns
 * [img_off[i], img_off[i + 1])).  svo_voc_transform: per feature the word, its weight and the ancestor `levelsup` levels
 * above the leaf (the direct index's node).  svo_voc_bow: an image's BowVector -- TF-IDF, L1-normalised, ascending word
 * order -- and per feature its direct-index node (-1: weight 0, the feature is in neither).                              */
typedef struct svo_voc svo_voc;
int svo_voc_create(svo_ctx *ctx, int k, int L, int n_nodes, const int *parent, const uint32_t *desc, const double *weight,
                   svo_voc **out);
int svo_voc_train(svo_ctx *ctx, const uint32_t *desc, const int *img_off, int n_images, int k, int L, uint64_t seed,
                  svo_voc **out);
int svo_voc_destroy(svo_voc *voc);
int svo_voc_info(const svo_voc *voc, int *k, int *L, int *n_nodes, int *n_words);
int svo_voc_export(const svo_voc *voc, int *parent, uint32_t *desc, double *weight, int *word_id);
int svo_voc_transform(svo_voc *voc, const uint32_t *desc, int n, int levelsup, int *word, double *weight, int *node, int mem);
int svo_voc_bow(svo_voc *voc, const uint32_t *desc, int n, int levelsup, int *words, double *values, int *n_words,
                int *node_per_feature);
/* The detector with the reference's scoring: once a vocabulary is set (before the first frame), entries are scored as
 * DBoW2 does -- BowVector per frame, inverted-file query with the L1 score (TemplatedDatabase::queryL1), normalisation by
 * the score against the previous frame (use_nss), alpha, islands, temporal window -- and the geometric check matches
 * through the direct index at di_levels (GEOM_DI, include/TemplatedLoopDetector.h:1005-1087).  The vocabulary must
 * outlive the detector.  Without one the detector keeps its vocabulary-free similarity (svo_lc_params.hamming_threshold). */
int svo_lc_set_vocabulary(svo_lc *lc, svo_voc *voc, int di_levels);
/* a frame given by its FEATURES instead of its image (a chunk-sharded run: every rank extracts svo_orb_extract on its own
 * frames, the 20 KB per frame travel to the rank that holds the database): xy n*2 floats, desc n*8 words               */
int svo_lc_submit_features(svo_lc *lc, const float *xy, const uint32_t *desc, int n, int mem);
/* n_frames frames by their features: `cap` slots per frame in xy (cap * 2 floats) and desc (cap * 8 words), n[g] of them
 * used; with a vocabulary 16 frames per set of launches (as svo_lc_submit_batch)                                        */
int svo_lc_submit_features_batch(svo_lc *lc, const float *xy, const uint32_t *desc, const int *n, int n_frames, int cap, int mem);
/* The same arrays as database entries that are NOT queries: no scoring, no verdict, nothing to collect.  A rank of a
 * chunk-sharded run fills its detector with every frame before its share this way (cheap: three launches per 16 frames),
 * then queues its own frames -- the detector's work is sharded like the front-end's (ros_stereo_slam_amd/chunked.py:
 * sharded_detect).  SVO_ERR_STATE while queued frames wait to be collected.                                          */
int svo_lc_fill_features_batch(svo_lc *lc, const float *xy, const uint32_t *desc, const int *n, int n_frames, int cap, int mem);
/* svo_lc_collect that also hands out what the verdict was formed from: the candidates of the database query in score
 * order (before removeLowScores) and the normalisation score; any pointer may be NULL                                    */
int svo_lc_collect_ex(svo_lc *lc, int *status, int *query, int *match, int *cand_id, double *cand_score, int cap,
                      int *n_cand, double *ns_factor);

/* ---- ANMS: adaptiveNonMaximalSuppresion(keypoints, numToKeep), src/ANMS.cpp:18-67 ------------ */
/* xy: n*2 floats, response: n floats (the reference's grid keypoints carry response 0; the
 * front-end passes the level-0 LK minimum eigenvalue).  out_idx: n ints capacity, receives the
 * input indices of the kept keypoints in the reference's output order (response-sorted).
 * count: host or device int following `mem`.                                                  */
int svo_anms(svo_ctx *ctx, const float *xy, const float *response, int n, int num_to_keep, int *out_idx,
             int *count, int mem);

/* ---- FAST: cv::FAST(image, kps, threshold, nonmaxSuppression), src/ANMS.cpp:76, and the FAST -> ANMS key-point source ----
 * The algorithm is the one tests/fast_numpy.py states; TYPE_9_16 only.  Grey is the image itself (c = 1) or
 * cvtColor's integer weights on B, G, R (c = 3).  A pixel (x, y), 3 <= x < w - 3 and 3 <= y < h - 3, is a corner when nine cyclically
 * contiguous pixels of the radius-3 ring are all > centre + threshold or all < centre - threshold.  Its score is the largest
 * threshold at which it is still one: over the 16 arcs of nine, the largest of min(ring - centre) and of min(centre - ring), minus
 * one.  nonmax_suppression != 0 keeps a corner whose score is strictly above the scores of its eight neighbours (0 for a neighbour
 * that is no corner or lies on the 3-pixel border; equal neighbours remove each other).  max_keypoints > 0 is
 * KeyPointsFilter::retainBest: every key point whose response is at or above the max_keypoints-th largest stays, ties included, so an
 * image can return more than max_keypoints.
 *
 * Output: key points in row-major order (y ascending, then x ascending); xy: the pixel as floats; response: the score with
 * suppression, 0 without (what cv::FAST leaves); KeyPoint::size 7 and angle -1 are constants and are not returned.
 *
 * svo_fast_detect_batch: n_images (1 ... 16) images of one size, w x h x c bytes each; images: a host array of host or device pointers
 * according to mem; xy / response hold n_images x cap entries, image i's at i * cap (response may be NULL); n: HOST ints in both
 * modes -- the call waits once, for the counts; score (optional: NULL, or n_images x w x h bytes following mem): the score plane
 * before suppression, 0 where no corner fires and on the border (diagnostics: it localises a parity failure).  An image with
 * w < 7 or h < 7 is legal and has no key points.  SVO_ERR_ARG: null ctx / images / an image / prm / xy / n, xy, response or n not
 * 4-byte aligned, c not 1 or 3, n_images outside 1 ... 16, cap < 1, w or h below 1 or above 16384, threshold outside 0 ... 255,
 * max_keypoints < 0.  SVO_ERR_CAPACITY: an image has more than cap key points -- every n[i] holds the needed count and the first
 * min(n[i], cap) key points of each image, in row-major order, are valid; nothing is written past cap.
 *
 * svo_fast_anms_batch: per image exactly what svo_fast_detect_batch, svo_anms(xy, response, n[i], num_to_keep) and a gather of xy /
 * response by the returned indices give, in ANMS's response-sorted order; n[i] is the kept count.  The key points stay on the
 * device in between (the host reads only the counts).  num_to_keep < 1: SVO_ERR_ARG.  When detection overflows cap the call returns
 * SVO_ERR_CAPACITY with the detector's counts in n and runs no ANMS (xy / response are then unspecified).  svo_anms has no bound
 * on n of its own: it is all-pairs, its time grows with n^2, and cap is the caller's limit.                                     */
typedef struct svo_fast_params {
    int threshold;          /* 10 (cv's default; the reference passes 1) */
    int nonmax_suppression; /* 1 */
    int max_keypoints;      /* 0 = all */
} svo_fast_params;
void svo_fast_default_params(svo_fast_params *p);
int svo_fast_detect_batch(svo_ctx *ctx, const uint8_t *const *images, int n_images, int w, int h, int c,
                          const svo_fast_params *prm, int cap, float *xy, float *response, uint8_t *score, int *n, int mem);
int svo_fast_anms_batch(svo_ctx *ctx, const uint8_t *const *images, int n_images, int w, int h, int c,
                        const svo_fast_params *prm, int num_to_keep, int cap, float *xy, float *response, int *n, int mem);

/* ---- goodFeaturesToTrack: cv::goodFeaturesToTrack / GFTTDetector (Shi-Tomasi min-eigenvalue or Harris corners) ----------------
 * The algorithm is the one tests/gftt_numpy.py states, points G1 ... G13.  Grey is the image itself (c = 1)
 * or cvtColor's integer weights on B, G, R (c = 3).  The corner measure is cornerMinEigenVal / cornerHarris with a 3 x 3 Sobel and a
 * block_size x block_size window, float arithmetic, nothing fused; corners are the 3 x 3 local maxima (plateaus whole) above
 * quality_level times the largest measure of the image -- of the pixels with a non-zero mask byte when a mask is given --, one
 * pixel inside the border, ordered by measure descending and row-major index descending among equals; min_distance >= 1 keeps, in
 * that order, the corners with no kept corner closer than min_distance (exactly the sequential greedy selection); max_corners > 0
 * keeps the first max_corners of them.
 *
 * svo_gftt_detect_batch: n_images (1 ... 16) images of one size, w x h x c bytes each; images: a host array of host or device
 * pointers according to mem; masks: NULL, or a host array of n_images pointers, each NULL or w x h bytes following mem; xy /
 * response hold n_images x cap entries, image i's at i * cap (response may be NULL), in acceptance order; response: the measure;
 * n: HOST ints in both modes.  w < 3 or h < 3 is legal and yields no corners.  SVO_ERR_ARG (nothing is written): null ctx / images /
 * an image / prm / xy / n, xy, response or n not 4-byte aligned, c not 1 or 3, n_images outside 1 ... 16, cap < 1, w or h below 1 or
 * above 16384, more than 2^24 interior pixels, (w - 2)(h - 2), in the images of one call (the candidate lists and the sort are
 * sized to that bound), block_size not odd in 3 ... 31, quality_level not in (0, 1] or NaN, negative or NaN min_distance, with
 * use_harris a k that is not finite as a float, mem neither SVO_MEM_HOST nor SVO_MEM_DEVICE.  SVO_ERR_CAPACITY: an image has more
 * than cap corners -- every n[i] holds the true count and the first min(n[i], cap) corners of each image are valid; nothing is
 * written past cap.
 *
 * svo_gftt_response: the measure of every pixel before thresholding, w x h floats following mem (any w, h >= 1).            */
typedef struct svo_gftt_params {
    int max_corners;      /* 1000; <= 0 = all */
    int block_size;       /* 3 */
    int use_harris;       /* 0 */
    int pad;              /* 0 */
    double quality_level; /* 0.01 */
    double min_distance;  /* 1.0 */
    double k;             /* 0.04 */
} svo_gftt_params;
void svo_gftt_default_params(svo_gftt_params *p);
int svo_gftt_detect_batch(svo_ctx *ctx, const uint8_t *const *images, const uint8_t *const *masks, int n_images, int w, int h, int c,
                          const svo_gftt_params *prm, int cap, float *xy, float *response, int *n, int mem);
int svo_gftt_response(svo_ctx *ctx, const uint8_t *image, int w, int h, int c, const svo_gftt_params *prm, float *eig, int mem);

/* ---- Star (CenSurE): xfeatures2d::StarDetector::create()->detect, the detector of the commented pair above
 * visualSLAM::stereoTriangulate (src/triangulation.cpp:79-80), with BriefDescriptorExtractor as its descriptor --------------------
 * The algorithm is the one tests/star_numpy.py states.  Grey is the image itself (c = 1) or cvtColor's
 * integer weights on B, G, R (c = 3).  For the size indices i of sizes0 = {1, 2, 3, 4, 6, 8, 11, 12, 16, 22, 23, 32, 45, 46, 64, 90,
 * 128}, r = sizes0[i] and t = r + r / 2, the star sum of a pixel is grey over the square |dx|, |dy| <= r plus grey over the diamond
 * |dx| + |dy| <= t (int32, exact).  svo_star_layout gives the number of (outer, inner) patterns in use, the largest size index and
 * the border = its t: the pattern count grows while the outer size is below max_size and the next outer star fits min(w, h), and
 * stops at the 12 patterns there are.  Inside the border a pixel's response is, over the patterns in order, the
 * float(inner) * (1.f / innerArea) - float(outer) * (1.f / outerArea) of the strictly largest magnitude (float32: two multiplies and
 * a subtraction) and its size the outer size of that pattern; outside, both are 0.  Suppression works on tiles of
 * (suppress_nonmax_size / 2 + 1)^2 pixels anchored at (border, border): a tile's strict maximum above response_threshold and its strict
 * minimum below -response_threshold are candidates; a candidate falls when another pixel within suppress_nonmax_size / 2 of it
 * (clipped to the image) is >= (<=) it, when its size is below 4, or when the line test fires on the response plane
 * (line_threshold_projected) or on the plane of pixels of its own size (line_threshold_binarized).
 *
 * Output: a tile's maximum before its minimum, tiles in row-major order; xy: the pixel as floats; size: the outer size; response:
 * the extremum, negative for minima; KeyPoint::angle -1 and octave 0 are constants and are not returned.
 *
 * svo_star_detect_batch: n_images (1 ... 16) images of one size, w x h x c bytes each; images: a host array of host or device pointers
 * according to mem; xy / size / response hold n_images x cap entries, image i's at i * cap (size and response may be NULL); n: HOST
 * ints in both modes -- the call waits once, for the counts.  A batch returns the bits of one call per image, host memory the bits
 * of device memory.  An image with no pixel inside the border is legal and has no key points.  SVO_ERR_ARG, nothing written: null ctx
 * / images / an image / prm / xy / n, xy, size, response or n not 4-byte aligned, c not 1 or 3, n_images outside 1 ... 16, cap < 1, w
 * or h below 1 or above 16384, max_size outside 3 ... 128, response_threshold < 0, a line threshold < 0, suppress_nonmax_size outside
 * 1 ... 31.  SVO_ERR_CAPACITY: 255 w h > 2^31 - 1 (the int32 tables could overflow; decided before any allocation, nothing
 * written), or an image has more than cap key points -- every n[i] then holds the needed count and the first min(n[i], cap) key
 * points of each image are valid; nothing is written past cap.
 *
 * svo_star_responses (diagnostics: it localises a parity failure): the response (w x h floats) and size (w x h int16) planes of one
 * image following mem, and the border as a HOST int.  Refusals as above; response 4-byte, size 2-byte aligned.
 *
 * svo_star_layout: host only, no context.  SVO_ERR_ARG for w or h outside 1 ... 16384 or max_size outside 3 ... 128; the outputs
 * may be NULL.  The defaults give 9 patterns, index 13 and border 69.                                                            */
typedef struct svo_star_params {
    int max_size;                 /* 45 */
    int response_threshold;       /* 30 */
    int line_threshold_projected; /* 10 */
    int line_threshold_binarized; /* 8 */
    int suppress_nonmax_size;     /* 5 */
} svo_star_params;
void svo_star_default_params(svo_star_params *p);
int svo_star_detect_batch(svo_ctx *ctx, const uint8_t *const *images, int n_images, int w, int h, int c,
                          const svo_star_params *prm, int cap, float *xy, float *size, float *response, int *n, int mem);
int svo_star_responses(svo_ctx *ctx, const uint8_t *image, int w, int h, int c, const svo_star_params *prm,
                       float *response, int16_t *size, int *border, int mem);
int svo_star_layout(int w, int h, int max_size, int *npatterns, int *max_idx, int *border);

/* ---- PnP-RANSAC: cv::solvePnPRansac(obj,img,K,0,rvec,tvec,false,its,thr,conf,inliers) --------- */
/* replaces src/keyFrameManagement.cpp:84 (100, 1.0, 0.99) and :88 (100, 8.0, 0.98).
 * obj: n*3 floats (world), img: n*2 floats, K4 = {fx, fy, cx, cy} (HOST doubles), no
 * distortion.  rvec/tvec/n_inliers/iters_run are HOST outputs in both memory modes (the caller
 * branches on them, src/keyFrameManagement.cpp:85, src/VisualSLAM.cpp:120); `inliers`
 * (n ints capacity, ascending indices) follows `mem`.  The call synchronises.                 */
int svo_pnp_ransac(svo_ctx *ctx, const float *obj, const float *img, int n, const double *K4,
                   int iterations, double reproj_err, double confidence, uint64_t seed, double *rvec,
                   double *tvec, int *inliers, int *n_inliers, int *iters_run, int mem);

/* ---- plain PnP: cv::solvePnP(obj, img, K, dist = 0, rvec, tvec) -------------------------------- */
/* SOLVEPNP_ITERATIVE without an extrinsic guess, the last rung of the older VO ladder
 * (src/bundleAdjust.cpp:470-477: "skipping RANSAC all together"): DLT over ALL n >= 6 points
 * (upstream's non-planar branch), then Levenberg-Marquardt on the reprojection error.  rvec / tvec /
 * rms (optional: root mean square reprojection error) are HOST outputs; obj / img follow `mem`.
 * SVO_ERR_STATE when the object points are planar (W[2] / W[1] < 1e-3 upstream; its homography
 * branch is not built) or degenerate.  The call synchronises.                                      */
int svo_solve_pnp(svo_ctx *ctx, const float *obj, const float *img, int n, const double *K4, double *rvec,
                  double *tvec, double *rms, int mem);

/* The pose ladder of the older visualOdometry::initSequence, src/bundleAdjust.cpp:462-480, on explicit
 * point sets: (obj_f, img_f, n_f) = the tracked set after the F-matrix filter, (obj_s, img_s, n_s) = the
 * status-filtered set that "retracking" without the filter yields.  rung (out): 0 = solvePnPRansac
 * (100, 4.0, 0.99) on the filtered set decided; 1 = fewer than 20 inliers or tvec.x > 1000, the same on
 * the status-filtered set; 2 = fewer than 10 (or tvec.x > 1000 again): plain solvePnP on the set last
 * used.  n_inliers: the last RANSAC's count.  Stage seeds seed + 1 / seed + 2.  SVO_ERR_TRACKING_LOST
 * when solvePnP has no solution (upstream: an uncaught cv::Exception).  svo_vo with
 * policy = SVO_POLICY_VO_LADDER runs this per frame.                                               */
int svo_pnp_ladder(svo_ctx *ctx, const float *obj_f, const float *img_f, int n_f, const float *obj_s,
                   const float *img_s, int n_s, const double *K4, uint64_t seed, double *rvec, double *tvec,
                   int *n_inliers, int *rung, int mem);

/* ---- motion BA: visualOdometry::BundleAdjust3d2d(points_2d, points_3d, K, R, t) ---------------- */
/* src/bundleAdjust.cpp:551-613 (unbuilt upstream, kept for completeness of the path the north-star
 * names): g2o Levenberg (BlockSolver<6,3>, dense pose solver) over ONE VertexSE3Expmap (R9 / t3:
 * world -> camera, as solvePnP returns them) and n FREE VertexSBAPointXYZ that are marginalised
 * (Schur-eliminated onto the 6x6 pose block, not fixed), one EdgeProjectXYZ2UV with identity
 * information per point, optimize(iterations = 10 upstream).  K4 = {fx, fy, cx, cy} HOST doubles;
 * upstream builds CameraParameters from K(0,0), K(0,2), K(1,2) only, so fy is NOT read (:588-590).
 * t3 (HOST, in/out) receives the optimised translation -- the only value upstream writes back
 * (:609-611).  Optional HOST outputs: R9_out, pts3d_out (n*3 doubles, the optimised points),
 * info[5] = {chi2 before, chi2 after, final lambda, iterations run, trials}.  pts2d (n*2 floats) /
 * pts3d (n*3 floats) follow `mem`.  The whole LM loop runs in one launch; the call synchronises.   */
int svo_ba_3d2d(svo_ctx *ctx, const float *pts2d, const float *pts3d, int n, const double *K4,
                const double *R9, double *t3, int iterations, double *R9_out, double *pts3d_out,
                double *info, int mem);

/* ---- windowed bundle adjustment: several poses, free points, mono and stereo observations ----- */
/* OURS in scope (upstream's README names it as future work), g2o's in arithmetic: Levenberg over
 * BlockSolver<6,3> with n_poses VertexSE3Expmap (poses12: R9 | t3 per pose, world -> camera; a pose
 * whose pose_fixed byte is non-zero is held) and n_points FREE, marginalised VertexSBAPointXYZ.
 * Observations are stored CSR by point: point i owns obs_start[i] .. obs_start[i+1]-1, each with
 * the index of the observing pose and (u, v, u_right).  u_right NaN: EdgeSE3ProjectXYZ, residual
 * (u - (fx x/z + cx), v - (fy y/z + cy)); else EdgeStereoSE3ProjectXYZ, which adds
 * u_right - (fx x/z + cx - bf/z).  Identity information.  huber_* > 0: g2o's RobustKernelHuber of
 * that delta on the observations of that kind (H and b scaled by rho', chi2 sums rho).
 * lambda0 = 1e-5 max|diag H| over pose and point blocks, at most ten trials per iteration, the
 * stopping rules of svo_ba_3d2d.  A point without observations is skipped and comes back
 * unchanged.  Refused with SVO_ERR_ARG, nothing written: n_poses outside 1..32, more than 16 or no
 * free poses, n_points < 1, an obs_pose out of range, an obs_start that decreases or does not
 * begin at 0, a point seen twice by one pose, a free pose with fewer than three observations,
 * iterations < 0, a negative Huber delta, a stereo observation with bf <= 0, a bad mem;
 * SVO_ERR_CAPACITY beyond 2^20 points or 2^28 observations.  poses12 / pose_fixed and the optional
 * outputs are HOST in both modes: pts3d_out n_points*3 doubles, obs_chi2_out the final e^T e of
 * every observation (no kernel applied), info[6] = {chi2 before, chi2 after, final lambda,
 * iterations run, trials, observations}.  Every sum runs in a fixed order: the result is the same
 * bit for bit on every run.  The host reads one small record per trial; the call synchronises.   */
typedef struct svo_ba_window_params {
    double fx, fy, cx, cy;   /* g2o EdgeSE3ProjectXYZ / EdgeStereoSE3ProjectXYZ read both focal lengths */
    double bf;               /* fx * baseline; read by stereo observations only                           */
    int    iterations;       /* default 10                                                                */
    double huber_mono;       /* 0 (default) = no kernel; else Huber delta on a 2-residual observation     */
    double huber_stereo;     /* 0 (default) = no kernel; else Huber delta on a 3-residual observation     */
} svo_ba_window_params;
void svo_ba_window_default_params(svo_ba_window_params *p);
int svo_ba_window(svo_ctx *ctx, const svo_ba_window_params *p, int n_poses, double *poses12,
                  const uint8_t *pose_fixed, int n_points, const float *pts3d, const int *obs_start,
                  const int *obs_pose, const float *obs_uvr, double *pts3d_out, double *obs_chi2_out,
                  double *info, int mem);

/* ---- the front-end frame loop: visualSLAM::initSequence, src/VisualSLAM.cpp:11-169 ----------- */
typedef struct svo_vo_params {
    double fx, fy, cx, cy;    /* include/visualSLAM.h:82-87 (KITTI 00-02)                      */
    double baseline;          /* include/visualSLAM.h:68, 0.54 m                               */
    int grid_step;            /* src/triangulation.cpp:89, 30 px                               */
    int anms_keep;            /* 0 = no ANMS (reference); else keep this many grid keypoints   */
    int keyframe_min_inliers; /* src/VisualSLAM.cpp:120, 200                                   */
    double f_thr_stereo;      /* src/tracking.cpp:34, 3.0 px                                   */
    double f_thr_temporal;    /* src/tracking.cpp:75, 1.0 px                                   */
    uint64_t seed;            /* RANSAC sampling seed; stage seeds are seed + 8*frame + stage  */
    int policy;               /* SVO_POLICY_SLAM (0, default): visualSLAM::initSequence,
                               * src/VisualSLAM.cpp:54-169.  SVO_POLICY_VO_LADDER (1): the older
                               * visualOdometry::initSequence, src/bundleAdjust.cpp:427-548 -- PnP-RANSAC
                               * at 4 px; < 20 inliers or tvec.x > 1000: again on the status-filtered
                               * set without the F-matrix filter; < 10: plain solvePnP; a stereo
                               * keyframe on EVERY frame; never shuts down.  Frame-by-frame entry
                               * points only (svo_vo_localize / update / track).                    */
    int pnp_retry_below;      /* src/keyFrameManagement.cpp:85, 10: fewer PnP inliers at 1 px -> the 8 px retry   */
    int pnp_lost_below;       /* src/keyFrameManagement.cpp:89, 10: fewer after the retry -> SHUTDOWN_FLAG        */
} svo_vo_params;
enum { SVO_POLICY_SLAM = 0, SVO_POLICY_VO_LADDER = 1 };
void svo_vo_default_params(svo_vo_params *p);

int svo_vo_create(svo_ctx *ctx, const svo_vo_params *params, int width, int height, int channels,
                  svo_vo **out);
int svo_vo_destroy(svo_vo *vo);
/* frame 0: stereoTriangulate(imL, imR), identity pose (src/VisualSLAM.cpp:22-41) */
int svo_vo_init(svo_vo *vo, const uint8_t *left, const uint8_t *right, int mem, int *n_points);
/* PerspectiveNpointEstimation + pose composition (src/VisualSLAM.cpp:64-74,
 * src/keyFrameManagement.cpp:73-94).  R9 (row-major) / t3: camera pose in the world.
 * Returns SVO_ERR_TRACKING_LOST where the reference sets SHUTDOWN_FLAG.                      */
int svo_vo_localize(svo_vo *vo, const uint8_t *left, int mem, double *R9, double *t3, int *n_inliers,
                    int *n_tracked);
/* keyframe rule and reference hand-over (src/VisualSLAM.cpp:93-152) with the pose the caller
 * settled on; force_keyframe is the reference's LC_FLAG.  `right` may be NULL when no
 * keyframe can be due.                                                                        */
int svo_vo_update(svo_vo *vo, const uint8_t *right, int mem, const double *R9, const double *t3,
                  int n_inliers, int force_keyframe, int *was_keyframe);
/* localize + update */
int svo_vo_track(svo_vo *vo, const uint8_t *left, const uint8_t *right, int mem, int force_keyframe,
                 double *R9, double *t3, int *n_inliers, int *was_keyframe, int *n_tracked);
/* The chunk runner: n_frames consecutive frames (lefts[i], rights[i]: one image pointer each,
 * all HOST or all DEVICE per `mem`) through the front-end without returning to the caller in
 * between -- exactly the result of n_frames calls of svo_vo_track(force_keyframe = 0).
 * Outputs per frame (host arrays, any may be NULL except R_out/t_out): R_out n*9, t_out n*3,
 * inliers_out, tracked_out, keyframe_out.  The frame policy (retry / lost thresholds, keyframe rule,
 * reference hand-over, pose composition) runs on the device; the host enqueues the whole chunk and
 * reads the per-frame records once.  pipeline != 0 (device images only) runs the chunk on four HIP
 * streams: filters + the tracking pass from the tracked set | PnP, the decision, the refinement and
 * a keyframe's hand-over | the stereo path of every frame, two frames ahead | pyramids, triangulation
 * and the tracking pass from the keyframe candidate's points, ahead as well (the process needs a
 * hardware queue per stream: GPU_MAX_HW_QUEUES >= 5);
 * results are identical.  Stops at tracking loss (SVO_ERR_TRACKING_LOST, *n_done frames completed).  */
int svo_vo_run_chunk(svo_vo *vo, const uint8_t *const *lefts, const uint8_t *const *rights, int n_frames,
                     int mem, int pipeline, double *R_out, double *t_out, int *inliers_out,
                     int *tracked_out, uint8_t *keyframe_out, int *n_done);
/* Precondition for jobs that share a context: identical image size, channels, grid step, ANMS budget,
 * intrinsics and baseline (their stages are sized as one launch); SVO_ERR_ARG otherwise.
 * Several independent chunks of a stream at once on ONE GPU (the per-GPU form of SURVEY.md 8e's
 * chunk sharding): every job is one svo_vo_run_chunk() call on its own host thread.  The
 * front-end's kernels are latency-bound (one wave per keypoint / hypothesis, a few hundred to a
 * few thousand waves per launch), so chunks on separate contexts interleave on the chip.  Jobs
 * whose svo_vo share one svo_ctx (at most 16, device images) form a group: one host thread
 * advances them in lock step and every stage (pyramids, pyramidal LK, filters, F-RANSAC, PnP,
 * keyframe path) goes out as ONE set of launches for all of them -- these kernels are latency
 * chains, so several jobs cost little more than one.
 * Every job gets exactly what svo_vo_run_chunk gives it alone.  rc / n_done are filled per job;
 * the return value is the first failing group's code other than SVO_ERR_TRACKING_LOST, else SVO_OK. */
typedef struct svo_chunk_job {
    svo_vo *vo;
    const uint8_t *const *lefts;
    const uint8_t *const *rights;
    int n_frames, mem, pipeline;
    double *R_out, *t_out;
    int *inliers_out, *tracked_out;
    uint8_t *keyframe_out;
    int n_done, rc;
    /* When both are set the chunk (re-)initialises on this stereo pair first -- svo_vo_init: stereo
     * keyframe, identity pose (every chunk of a sharded stream starts like frame 0,
     * src/VisualSLAM.cpp:22-41) -- and lefts / rights are the frames AFTER it.  The initialisations
     * of the jobs of one group go out as one set of launches.  NULL: continue from the current state. */
    const uint8_t *init_left, *init_right;
    int n_init_points; /* out: points of the initial keyframe (when initialised here) */
} svo_chunk_job;
int svo_vo_run_chunks(svo_chunk_job *jobs, int n_jobs);
/* the current reference point set (2-D in the reference image, 3-D world) */
int svo_vo_get_reference(svo_vo *vo, float *ref2d, float *ref3d, int cap, int *n, int mem);
int svo_vo_capacity(const svo_vo *vo);
/* Where a frame of a PIPELINED chunk (svo_vo_run_chunk, pipeline != 0) spends its time: with stamps enabled a run of more
 * than 40 frames writes the device's 100 MHz clock between its stages (one-lane launches on the four streams: they cost a
 * few per cent, so a timed run leaves them off) and keeps the mean intervals over the middle of the run, in microseconds:
 *   [0] frame period on the main stream  = [1] filters + [2] tracking launch + [3] waiting for the decision
 *   [4] PnP stream starts after the filters, [5] from there to the keyframe decision, [6] a keyframe's refinement + hand-over
 *   [7] stereo stream starts after the tracking launch, [8] stereo path
 * (the per-frame body of src/VisualSLAM.cpp:54-169 as the four streams run it).  *n_frames = frames averaged (0: none yet). */
enum { SVO_STAGE_COUNT = 9 };
int svo_vo_set_stage_stamps(svo_vo *vo, int enable);
int svo_vo_get_stage_us(const svo_vo *vo, double *us, int cap, int *n_frames);
/* `colors` of the last keyframe (getColors(imL, its 2-D points): B, G, R as floats per point,
 * include/monoUtils.h:180-193, src/triangulation.cpp:139-140), point for point with svo_vo_get_keyframe_cloud:
 * what src/VisualSLAM.cpp:125-136 pushes into colorHistory.  Gathered by the triangulation launch itself. */
int svo_vo_get_keyframe_colors(svo_vo *vo, float *bgr, int cap, int *n, int mem);

/* ---- the chunk-sharded batch across GPUs: its one exchange step ------------------
 * The frame loop is sequential in time (src/VisualSLAM.cpp:54-200: frame n consumes frame n-1's
 * surviving points), so a batch shards across GPUs only as contiguous chunks that re-initialise at
 * their first frame and end ON the next chunk's first frame.  One process per GPU, each with its own
 * svo_ctx; the ranks exchange their chunk-boundary poses ONCE -- 12 doubles per chunk, [R row-major | t]
 * of the chunk's last frame in the chunk's own frame -- with an RCCL all-gather, prefix-compose them
 * and rebase their poses; the rebased trajectories then feed one pose graph (svo_pg_*).
 * librccl is loaded at run time; without it these calls return SVO_ERR_STATE.
 *   id128: 128 bytes (ncclUniqueId) made by ONE rank and carried to the others by the host's own means. */
typedef struct svo_shard_comm svo_shard_comm;
int svo_shard_unique_id(void *id128);
int svo_shard_comm_create(svo_ctx *ctx, int rank, int nranks, const void *id128, svo_shard_comm **out);
int svo_shard_comm_destroy(svo_shard_comm *comm);
int svo_shard_comm_rank(const svo_shard_comm *comm);
int svo_shard_comm_size(const svo_shard_comm *comm);
/* local12: this rank's n_chunks x 12 doubles (host); all12: nranks x n_chunks x 12 (host), rank-major */
int svo_shard_allgather_boundaries(svo_shard_comm *comm, const double *local12, int n_chunks, double *all12);
/* the same collective for plain bytes (the sharded loop detector's features, 20 KB per frame): bytes_per_rank bytes of
 * every rank to every rank, rank-major; the same count on every rank; host arrays                                     */
int svo_shard_allgather_bytes(svo_shard_comm *comm, const void *local, size_t bytes_per_rank, void *all);
/* boundaries of ALL chunks in global order -> the global pose of every chunk's first frame
 * (identity, B0, B0 B1, ...); host arithmetic, no communicator needed */
int svo_shard_prefix_starts(const double *boundaries12, int n_total, double *starts12);
/* chunk-local poses (n x 12, relative to the chunk's first frame) -> global poses, in place */
int svo_shard_rebase(const double *start12, double *poses12, int n);

/* ---- the keyframe map and its re-projection: visualSLAM::updateOdometry ------------------------ */
/* src/optimizationStuff.cpp:17-47 over keyFrameHistory (src/VisualSLAM.cpp:152-166,
 * include/visualSLAM.h:47-54).  The camera-frame clouds of the stored records stay in HBM;
 * svo_map_update re-transforms ALL of them in one launch with [R_old | t_new]: the record's own,
 * un-optimised rotation and the optimised translation of trajectory entry `traj_index` (:29-41).    */
typedef struct svo_map svo_map;
int svo_map_create(svo_ctx *ctx, svo_map **out);
int svo_map_destroy(svo_map *map);
/* keyFrameHistory.emplace_back(kf): kf.R = R9, kf.t = t3 (camera in the world), kf.ref3dCoords =
 * xyz_cam (n*3 floats, camera frame: the `untransformed` cloud; follows `mem`), kf.retrack; traj_index =
 * the record's index into the trajectory updateOdometry receives (upstream: the frame number).  The
 * record's world cloud is placed at once as insertKeyFrames does (src/keyFrameManagement.cpp:20-30).  */
int svo_map_add_keyframe(svo_map *map, int traj_index, const double *R9, const double *t3, const float *xyz_cam,
                         int n, int retrack, int mem);
int svo_map_num_keyframes(const svo_map *map);
/* updateOdometry(T): t3s = the translations of T (n_poses*3 HOST doubles, e.g. columns 0-2 of
 * svo_pg_get_estimates).  Asynchronous on the context's stream.                                      */
int svo_map_update(svo_map *map, const double *t3s, int n_poses);
/* mapHistory: the world clouds of the records with retrack, in order, back to back (xyz_world:
 * cap_points*3 floats, follows `mem`) and their sizes (counts, HOST).  Both may be NULL to query the
 * totals (*n_points, *n_keyframes: HOST).                                                           */
int svo_map_get_points(svo_map *map, float *xyz_world, size_t cap_points, int *counts, int cap_keyframes,
                       size_t *n_points, int *n_keyframes, int mem);
/* the camera-frame cloud of the front-end's LAST keyframe (`untransformed`, src/keyFrameManagement.cpp:18),
 * valid until the next keyframe; xyz_cam: cap*3 floats following `mem`.                              */
int svo_vo_get_keyframe_cloud(svo_vo *vo, float *xyz_cam, int cap, int *n, int mem);

/* ---- SE3 pose graph: globalPoseGraph, include/poseGraph.h:36-179 ------------------------------ */
/* Poses are 7 doubles: tx ty tz qx qy qz qw (the VERTEX_SE3:QUAT order of g2o).  All pose and
 * chi2 arrays of this group are HOST memory: the graph is built on the host one vertex per frame
 * (src/optimizationStuff.cpp:3-15) and optimised on the device.                                */
int svo_pg_create(svo_ctx *ctx, svo_posegraph **out); /* includes initializeGraph()             */
int svo_pg_destroy(svo_posegraph *pg);
/* initializeGraph, poseGraph.h:69-84: vertex 0 = identity, fixed */
int svo_pg_initialize(svo_posegraph *pg);
/* augmentNode(localT, globalT), poseGraph.h:87-111: new vertex with estimate globalT and an edge
 * from the previous vertex whose measurement is prev^-1 * cur of the CURRENT estimates (localT is
 * never read by the reference and is not a parameter here) */
int svo_pg_augment_node(svo_posegraph *pg, const double *pose7);
/* addLoopClosure(T, fromID), poseGraph.h:113-126: edge(previous vertex -> vertex fromID) with
 * IDENTITY measurement (T is unused by the reference) */
int svo_pg_add_loop_closure(svo_posegraph *pg, int from_id);
/* n frames in one call: for i = 0 .. n-1, svo_pg_add_loop_closure(closure_from[i]) if closure_from && closure_from[i] >= 0,
 * then svo_pg_augment_node(pose7 + 7 i) -- the staging order of the reference (src/optimizationStuff.cpp:3-15,58-63).        */
int svo_pg_augment_nodes(svo_posegraph *pg, int n, const double *pose7, const int *closure_from);
/* globalOptimize, poseGraph.h:128-138: `iters` Gauss-Newton iterations (the reference: 10).
 * chi2 (optional, iters+1 doubles): the error before each iteration and after the last.
 * SVO_ERR_STATE: the normal matrix was not positive definite (the graph is left as it was);
 * SVO_ERR_ARG: more than about 1600 SEPARATORS = distinct loop-closure endpoints + one regular separator per 104
 * vertices of a run without one (the separator solve keeps its vector in one workgroup's LDS): a chain of about 170 000
 * vertices reaches that without a single closure; KITTI 00 (4541 vertices, < 100 endpoints with the reference's 100-frame
 * cooldown) uses about 120. */
int svo_pg_optimize(svo_posegraph *pg, int iters, double *chi2);
/* Iterative refinement of every Gauss-Newton step's linear solve (round 5): `passes` more solves with the SAME elimination,
 * each for the residual rneg - H dx of the step so far, formed in double-double on the device.  0 (the default; also
 * SVO_PG_REFINE in the environment at svo_pg_create) is g2o's single solve.  The normal matrix of a long chain with
 * identity information is conditioned like the square of its length (4541 vertices: ~1e8): one solve leaves the step
 * good to 1e-9 ... 3e-8 of the trajectory's extent, one refinement pass to < 1e-10, measured against a sparse LU refined
 * with 80-bit residuals (tests/pg_arbiter.py).  Each pass costs one more elimination (+0.25 ms per iteration at 4541 / 40). */
int svo_pg_set_refinement(svo_posegraph *pg, int passes);
int svo_pg_num_vertices(const svo_posegraph *pg);
int svo_pg_num_edges(const svo_posegraph *pg);
int svo_pg_get_estimates(const svo_posegraph *pg, double *pose7_out);
int svo_pg_get_edge(const svo_posegraph *pg, int e, int *from, int *to, double *meas7);
/* saveStructure, poseGraph.h:140-179: VERTEX_SE3:QUAT / EDGE_SE3:QUAT text */
int svo_pg_write_g2o(const svo_posegraph *pg, const char *path);
/* the inverse: replace the graph by a .g2o file (VERTEX_SE3:QUAT / EDGE_SE3:QUAT / FIX 0; the
 * information matrices are ignored -- the reference leaves them at identity, poseGraph.h:102,122) */
int svo_pg_read_g2o(svo_posegraph *pg, const char *path);
/* ---- per-edge information matrices and measured loop closures ---------------------------------
 * An edge's error is e = [t ; s q_xyz] of Z^-1 Xi^-1 Xj (g2o's order: translation first); its information Om is a symmetric
 * positive-definite 6 x 6 matrix in those coordinates, passed as the 21 numbers of its upper triangle, row-major (what an
 * EDGE_SE3:QUAT line carries).  chi2 = e^T Om e, H = J^T Om J, b = J^T Om e.  A graph on which no information other than
 * the identity was ever set is optimised by the same kernel, to the same bits, as before these calls existed; the exact
 * identity is stored as "none".  SVO_ERR_ARG, with a text that names the edge and the graph left as it was: an entry that
 * is not finite, or a matrix whose 6 x 6 Cholesky factorisation meets a pivot <= 0.                                    */
/* edge(previous vertex -> vertex from_id) with measurement meas7 (tx ty tz qx qy qz qw, quaternion normalised on entry;
 * NULL = identity = svo_pg_add_loop_closure) and information info21 (NULL = I).
 * What addLoopClosure(T, fromID) would do if it read its T (poseGraph.h:113-126; dump.cpp:331-348 produces that T). */
int svo_pg_add_loop_closure_measured(svo_posegraph *pg, int from_id, const double *meas7, const double *info21);
int svo_pg_set_edge_information(svo_posegraph *pg, int e, const double *info21);   /* NULL resets to identity */
int svo_pg_get_edge_information(const svo_posegraph *pg, int e, double *info21);  /* identity when none stored */
/* svo_pg_read_g2o that KEEPS the information of EDGE_SE3:QUAT lines: a line carries none (identity) or exactly 21 numbers,
 * any other count is SVO_ERR_ARG with the line number.  svo_pg_write_g2o writes stored information as %.17g and, for an
 * edge that stores none, the integers 1 / 0 of the identity.                                                         */
int svo_pg_read_g2o_info(svo_posegraph *pg, const char *path);
/* ---- robust kernels on edges, and pruning ------------------------------------------------------
 * An edge that carries a kernel enters a Gauss-Newton iteration as w Om instead of Om, in H and in b alike, with
 * w = rho'(c) at c = chi2 = e^T Om e of the edge at that iteration's estimates: iteratively re-weighted least squares, g2o's
 * robustInformation without the second-order term (commented out upstream).  The kinds and their weights are g2o's
 * robust_kernel_impl.h (src/bundleAdjust.cpp:19 includes it) and Open3D's line process -- FROM MEMORY, VERIFY:
 *   HUBER(d):          c <= d^2: rho = c, w = 1;  else rho = 2 d sqrt(c) - d^2, w = d / sqrt(c)
 *   CAUCHY(d):         rho = d^2 log(1 + c / d^2), w = 1 / (1 + c / d^2)
 *   DCS(phi):          s = 2 phi / (phi + c);  s >= 1: rho = c, w = 1;  else rho = s^2 c, w = s^2 -- g2o's weight here is NOT the
 *                      derivative of its rho; it is reproduced as it stands
 *   GEMAN_MCCLURE(mu): rho = mu c / (mu + c), w = l = (mu / (mu + c))^2 -- the line-process weight of Open3D's global
 *                      optimisation for an `uncertain` edge (src/ROSslam.py:57 adds every closure as one)
 * chi2[] of svo_pg_optimize stays the unweighted sum of e^T Om e (g2o's activeChi2).  A graph that stores no kernel is
 * optimised by the same kernels, to the same bits, as before these calls existed; so is one whose weights are all 1.   */
#define SVO_PG_ROBUST_NONE          0
#define SVO_PG_ROBUST_HUBER         1
#define SVO_PG_ROBUST_CAUCHY        2
#define SVO_PG_ROBUST_DCS           3
#define SVO_PG_ROBUST_GEMAN_MCCLURE 4
/* SVO_ERR_ARG, the graph unchanged: e outside the edges, an unknown kind, a delta that is not finite and positive (NONE takes
 * any).  The getter gives NONE and 0 for an edge that carries none; either output may be NULL.                       */
int svo_pg_set_robust_kernel(svo_posegraph *pg, int e, int kind, double delta);
int svo_pg_get_robust_kernel(const svo_posegraph *pg, int e, int *kind, double *delta);
/* The kernel of every edge svo_pg_add_loop_closure, svo_pg_add_loop_closure_measured and svo_pg_augment_nodes add AFTER this
 * call (NONE when the graph is created, and again after svo_pg_initialize and the .g2o readers).  Odometry edges never get one. */
int svo_pg_set_loop_closure_kernel(svo_posegraph *pg, int kind, double delta);
/* Per edge at the current estimates: chi2 = e^T Om e, the weight w and rho of its kernel (1 and chi2 without one); ne HOST
 * doubles each, any of the three may be NULL.  No blocks are formed; the call waits once.                             */
int svo_pg_edge_residuals(svo_posegraph *pg, double *chi2, double *weight, double *rho);
/* The weights the LAST linearisation of the last svo_pg_optimize stored in its per-edge records (ne HOST doubles), i.e. at
 * the estimates that call returned.  SVO_ERR_STATE when that solve used no kernel or the graph has changed since.      */
int svo_pg_linearization_weights(svo_posegraph *pg, double *weight);
/* Evaluates w at the current estimates and removes every edge that carries a kernel, does not join consecutive vertices
 * and has w < threshold (strict).  The other edges keep their order; measurements, information matrices and kernels move
 * with them.  removed (cap HOST ints, may be NULL with cap 0): the former indices, ascending; *n_removed (optional): their
 * count, also when the call refuses.  SVO_ERR_CAPACITY: cap is below the count; SVO_ERR_STATE: a vertex would no longer be
 * reachable from vertex 0; SVO_ERR_ARG: a NaN threshold -- nothing is removed in any of these.  After a removal the next
 * svo_pg_optimize uploads the graph and builds the elimination structure again.                                        */
int svo_pg_prune_edges(svo_posegraph *pg, double threshold, int *removed, int cap, int *n_removed);

/* ---- the measurement of a loop closure: getLCMeasurement, dump.cpp:331-348 -------------------- */
typedef struct svo_closure_params {
    double f_thr;       /* 1.0: PyrLKtrackFrame2Frame's filter, src/tracking.cpp:75; <= 0 skips it */
    int pnp_iterations; /* 100, 0.1, 0.999: dump.cpp:340 */
    double pnp_reproj_err, pnp_confidence;
    uint64_t seed;
} svo_closure_params;
void svo_closure_default_params(svo_closure_params *p);
/* newest: the newest frame's image with its n points (xy2 in that image, xyz3 in THAT CAMERA's frame); matched: the image of the
 * matched frame.  LK newest -> matched, compaction by status, F-matrix RANSAC at f_thr (confidence 0.99, seed + 1), compaction
 * by mask, PnP-RANSAC (seed + 2), then Rodrigues, R <- R^T, t <- -R tvec: meas7 = X_newest^-1 * X_matched, i.e. the measurement
 * of the edge svo_pg_add_loop_closure_measured adds.  The quaternion of R (row-major r00 .. r22), in this order of operations:
 *   tr = r00 + r11 + r22;
 *   tr > 0:                 s = 2 sqrt(tr + 1),            q = ((r21 - r12) / s, (r02 - r20) / s, (r10 - r01) / s, s / 4)
 *   else r00 largest:       s = 2 sqrt(1 + r00 - r11 - r22), q = (s / 4, (r01 + r10) / s, (r02 + r20) / s, (r21 - r12) / s)
 *   else r11 > r22:         s = 2 sqrt(1 + r11 - r00 - r22), q = ((r01 + r10) / s, s / 4, (r12 + r21) / s, (r02 - r20) / s)
 *   else:                   s = 2 sqrt(1 + r22 - r00 - r11), q = ((r02 + r20) / s, (r12 + r21) / s, s / 4, (r10 - r01) / s)
 * ("r00 largest": r00 > r11 and r00 > r22), divided by sqrt(((x x + y y) + z z) + w w), negated if w < 0 (so w >= 0).
 * images / xy2 / xyz3 follow `mem`; K4 / p / meas7 / n_tracked (points PnP saw) / n_inliers: HOST.  The call synchronises.
 * SVO_ERR_TRACKING_LOST below 6 PnP inliers (meas7 untouched; the counts are written).                             */
int svo_closure_measure(svo_ctx *ctx, const uint8_t *newest, const uint8_t *matched, int w, int h, int c, const float *xy2,
                        const float *xyz3, int n, const double *K4, const svo_closure_params *p, double *meas7,
                        int *n_tracked, int *n_inliers, int mem);

/* ---- point-to-plane ICP between clouds and the information of the edge it yields ---------------
 * PoseGraphOptimize of the Python prototype (src/ROSslam.py:34-73): pairwiseRegistration = a coarse and a fine
 * open3d registration_icp(TransformationEstimationPointToPlane) and get_information_matrix_from_point_clouds.
 * Open3D is recalled, not linked: tests/icp_numpy.py states every recalled point and every choice of ours, and the
 * device is held to that restatement bit for bit.
 *
 * svo_cloud: a resident TARGET cloud of 1 <= n <= 4194304 float32 points with its search index (Morton order and the
 * 64-way box hierarchy of svo_sor_filter_large), built once at creation and reused by every search: each ICP
 * iteration, both passes, the information matrix and the normals.  A point with a non-finite coordinate is
 * SVO_ERR_ARG whose text names the first offending index (indices are part of the results, nothing is dropped).
 * xyz follows `mem`; the call synchronises.  Normals are n x 3 DOUBLES in the points' order (Open3D's type).      */
typedef struct svo_cloud svo_cloud;
int svo_cloud_create(svo_ctx *ctx, const float *xyz, int n, int mem, svo_cloud **out);
int svo_cloud_destroy(svo_cloud *cloud);
int svo_cloud_size(const svo_cloud *cloud);
int svo_cloud_has_normals(const svo_cloud *cloud);
int svo_cloud_set_normals(svo_cloud *cloud, const double *normals, int mem);
int svo_cloud_get_normals(svo_cloud *cloud, double *normals, int mem); /* SVO_ERR_STATE without normals */
/* The k nearest points of every point, itself included (KDTreeSearchParamKNN), ordered by (d2, index); d2 =
 * (dx dx + dy dy) + dz dz in double.  idx_out: n x k ints following `mem`, rows shorter than k (n < k) end in -1.
 * k in 3 .. 64, else SVO_ERR_ARG.  Exact: equal to brute force over the whole cloud.                               */
int svo_cloud_knn(svo_cloud *cloud, int k, int *idx_out, int mem);
/* estimate_normals(KDTreeSearchParamKNN(knn)), knn in 3 .. 64 (Open3D's default: 30): per point the mean and the
 * covariance sum of its neighbours in double, in the neighbour order above; the eigenvector of the smallest
 * eigenvalue by 8 cyclic Jacobi sweeps, normalised, sign as the solver leaves it (never oriented); a point with
 * fewer than 3 neighbours, or a zero / non-finite vector, gets (0, 0, 1).  Asynchronous on the context's stream.   */
int svo_cloud_estimate_normals(svo_cloud *cloud, int knn);

typedef struct svo_icp_params {
    int max_iteration;       /* 30: ICPConvergenceCriteria's defaults */
    double relative_fitness; /* 1e-6 */
    double relative_rmse;    /* 1e-6 */
} svo_icp_params;
void svo_icp_default_params(svo_icp_params *p);
/* The correspondences of T src in the target: per source point the nearest target point (distance as above, the
 * lowest target index on a tie) when d2 < max_dist^2, else -1; fitness = n_corr / n_src, rmse = sqrt(sum d2 / n_corr)
 * (0 without correspondences).  T16: 4 x 4 row-major HOST doubles, source coordinates -> target frame.  corr_out
 * (optional, n_src ints) and src_xyz follow `mem`; the scalars are HOST.  The call synchronises.                  */
int svo_icp_correspondences(svo_ctx *ctx, const float *src_xyz, int n_src, svo_cloud *target, double max_dist,
                            const double *T16, int *corr_out, double *fitness, double *rmse, int mem);
/* J^T J (upper triangle, row-major, 21 HOST doubles) and J^T r (6) of ONE point-to-plane step at T16: r = (s - t) . n,
 * J = [s x n, n], summed over the correspondences on the fixed tree of DESIGN.md section 10i.  SVO_ERR_STATE when the
 * target has no normals.                                                                                          */
int svo_icp_normal_equations(svo_ctx *ctx, const float *src_xyz, int n_src, svo_cloud *target, double max_dist,
                             const double *T16, double *JtJ21, double *Jtr6, int *n_corr, int mem);
/* registration_icp(source, target, max_dist, T_init, TransformationEstimationPointToPlane(), criteria).  The solve,
 * the update of T and the convergence test run on the device: every iteration is queued at once, iterations after
 * the stop leave at once, and the host waits once.  iterations: updates applied (1 .. max_iteration).  corr_out
 * (optional, follows `mem`): the correspondences of the final T.  SVO_ERR_STATE: the target has no normals;
 * SVO_ERR_ARG: max_dist <= 0, n_src < 1, max_iteration < 1.                                                       */
int svo_icp_point_to_plane(svo_ctx *ctx, const float *src_xyz, int n_src, svo_cloud *target, double max_dist,
                           const double *T_init16, const svo_icp_params *params, double *T_out16, double *fitness,
                           double *rmse, int *iterations, int *corr_out, int mem);
/* get_information_matrix_from_point_clouds: Lambda = sum G^T G over the correspondences of T src at max_dist, G =
 * [-[t]x | I3] at the TARGET point t: 6 x 6 row-major, rotation first, then translation.  No normals needed.       */
int svo_icp_information(svo_ctx *ctx, const float *src_xyz, int n_src, svo_cloud *target, double max_dist,
                        const double *T16, double *info36, int *n_corr, int mem);
/* pairwiseRegistration: ICP at dist_coarse from the identity, ICP at dist_fine from its result, the information at
 * dist_fine; one index, one wait.  fitness / rmse / iterations (optional): [2] = coarse, fine.                    */
int svo_icp_pairwise(svo_ctx *ctx, const float *src_xyz, int n_src, svo_cloud *target, double dist_coarse,
                     double dist_fine, const svo_icp_params *params, double *T_out16, double *info36, double *fitness2,
                     double *rmse2, int *iterations2, int *n_corr, int mem);
/* Host code.  Lambda is the information of a LEFT perturbation T <- exp([w ; v]) T in the target frame; an edge whose
 * measurement is Z = T has the error e = [t ; s q_xyz] of Z^-1 Xi^-1 Xj = M [w ; v] to first order, M = the adjoint of
 * T^-1 reordered to translation first with the rotation rows halved.  info21 = the upper triangle, row-major, of
 * M^-T Lambda M^-1 (M^-1 = [0, 2R ; R, 2 [t]x R] in closed form), as svo_pg_set_edge_information takes it.
 * For svo_pg_add_loop_closure_measured: source = the matched keyframe's cloud, target = the newest frame's, each in
 * its own camera frame; T = X_newest^-1 X_matched is that call's meas7.                                            */
int svo_icp_edge_information(const double *info36, const double *T16, double *info21);
/* T16 -> tx ty tz qx qy qz qw by the quaternion formula stated at svo_closure_measure (host code) */
int svo_icp_meas7(const double *T16, double *meas7);

/* ---- data formats either side of the path (host code, no GPU work) -------------------------- */
/* KITTI odometry pose files: one pose per line, 12 numbers = the 3x4 [R|t]
 * row-major, camera-to-world.  Rt12: capacity*12 doubles; *n = poses in the file.                */
int svo_io_read_kitti_poses(const char *path, double *Rt12, int capacity, int *n);
int svo_io_write_kitti_poses(const char *path, const double *R9s, const double *t3s, int n);
/* trajectory.csv of the reference (createData / appendData, include/monoUtils.h:23-49): header
 * "Idx,Xm,Ym,Zm,Xgt,Ygt,Zgt,Const" when create != 0, then rows of 8 floats each followed by ','  */
int svo_io_trajectory_csv(const char *path, const float *rows8, int n_rows, int create);
/* Sequence input: visualSLAM::loadImageL / loadImageR (src/keyFrameManagement.cpp:48-71) =
 * sprintf(FileName, pattern, iter) + cv::imread(FileName) -> BGR8.  pattern: the reference's
 * "<dir>/image_2/%0.6d.png"-style string (src/VisualSLAM.cpp:220-222) with exactly one integer
 * conversion.  Decoded here, recognised by content: PNG -- what KITTI ships; every colour type and bit depth, Adam7
 * interlace, CRC and Adler-32 checked; the library's own inflate, no libpng / zlib dependency (csrc/png.hip) -- and
 * binary PGM (P5) / PPM (P6), 8 bit.  channels = 3 gives what imread's default IMREAD_COLOR gives (B,G,R interleaved; a
 * grey file replicated; alpha dropped; 16-bit samples by their high byte), 1 a grey image.  A missing file is
 * SVO_ERR_ARG with the reference's "failed to fetch frame, check the paths" text.                */
int svo_io_format_path(char *out, int cap, const char *pattern, int iter);
int svo_io_image_info(const char *path, int *w, int *h, int *c);
int svo_io_read_image(const char *path, int channels, uint8_t *out, size_t cap_bytes, int *w, int *h);
int svo_io_load_frame(const char *pattern, int iter, int channels, uint8_t *out, size_t cap_bytes, int *w, int *h);
/* a PNG held in memory (a ROS sensor_msgs/CompressedImage payload, a file the host has read itself) */
int svo_io_decode_png(const uint8_t *data, size_t n_bytes, int channels, uint8_t *out, size_t cap_bytes, int *w, int *h);
/* the inverse (tests, dataset conversion): BGR / grey -> PPM / PGM */
int svo_io_write_image(const char *path, const uint8_t *img, int w, int h, int channels);
/* getAbsoluteScale(frame_id, X, Y, Z), include/monoUtils.h:130-158: position of frame_id - 1 in a
 * KITTI pose file and the distance frame_id - 1 -> frame_id (the reference's ground-truth reader) */
int svo_io_absolute_scale(const char *poses_path, int frame_id, double *x_prev, double *y_prev, double *z_prev,
                          double *scale);
/* absolute trajectory error: RMSE of |t_est - t_gt| (no alignment: both start at the identity)   */
int svo_eval_ate_rmse(const double *t3_est, const double *t3_gt, int n, double *rmse);
/* relative pose error over frame pairs (i, i + delta): E = (Qi^-1 Qj)^-1 (Pi^-1 Pj); RMSE of the
 * translation norm and of the rotation angle (rad).  R9s row-major camera-to-world.              */
int svo_eval_rpe(const double *R9_est, const double *t3_est, const double *R9_gt, const double *t3_gt, int n,
                 int delta, double *trans_rmse, double *rot_rmse);
/* the map / pose messages of rosPublish (src/rosFuncs.cpp:41-98): points with -z > 500 are
 * skipped, the rest go out as (x, z, -y) * 0.1 with colour (r, g, b) = (c.z, c.y, c.x);
 * returns the number written.  xyz_out: n*3 floats, rgb_out: n*3 bytes (may be NULL).           */
int svo_ros_map_points(const float *xyz, const float *bgr, int n, float *xyz_out, uint8_t *rgb_out);
/* pose message: position (0.1 t0, 0.1 t2, -0.1 t1); orientation from the reference's Rmat2Quat
 * (include/monoUtils.h:215-227: the Rodrigues vector's components used as X, Y, Z angles) with
 * the component shuffle of src/rosFuncs.cpp:88-91.  pos3 / quat4 (x, y, z, w).                   */
int svo_ros_pose(const double *R9, const double *t3, double *pos3, double *quat4);
/* binary little-endian PLY (x y z float, red green blue uchar), the file SHUTDOWN writes at
 * src/rosFuncs.cpp:63-67 (PCL's extra camera element is not written)                            */
int svo_io_write_ply(const char *path, const float *xyz, const uint8_t *rgb, int n);

#ifdef __cplusplus
}
#endif
#endif
