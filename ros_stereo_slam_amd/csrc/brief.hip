// brief.hip -- OpenCV 3.2's xfeatures2d::BriefDescriptorExtractor, the descriptor of StereoProcess::stereoTriangulate
// (src/StereoCV.cpp:66-75: SIFT::create(20000)->detect, brief->compute, convertTo(CV_32F), BFMatcher).
//
// The algorithm is stated operation by operation in tests/brief_numpy.py (points B1 ... B7 as recalled from upstream, OURS-1
// where upstream would read past its integral image) and DESIGN.md section 10e; everything here is integer arithmetic apart
// from the two roundings of a key point's coordinates, which are done in double as the C++ expressions do them.
//
// Stages, all on the context's stream, blockIdx.y = image of the batch, one host wait (for the counts):
//   1. integral image: a workgroup per row scans the grey row (wave scans joined through LDS, a carry between the strips of
//      256 pixels), then a thread per column adds the rows up -- coalesced across the row.  int32, exact: no order dependence.
//   2. filter: runByImageBorder(28) + OURS-1 as a byte mask, compacted in order by the wave-segment compaction of geometry.hip.
//   3. descriptors: one wavefront per kept key point; the test table is staged once per workgroup into LDS, lane l evaluates
//      tests l, l + 64, ..., the 64 outcomes of a round come together in a ballot and the descriptor leaves in one byte store
//      per lane.
#include <cmath>
#include <cstring>

#include "svo_internal.h"
#include "brief_pattern.hip.h"
#include "scan_ops.hip.h"

namespace {

#include "feature_batch.hip.h"
#include "integral_scan.hip.h"

constexpr int BRIEF_MAXBATCH = IMAGE_MAXBATCH, BRIEF_BORDER = 28, BRIEF_HALF_PATCH = 24;
constexpr int BRIEF_WAVES = 4;       // key points a workgroup of the descriptor kernel works on at a time
constexpr int BRIEF_MAXGRID = 2048;  // its workgroups per image: 8 per CU, each wave walks on with that stride

struct BriefCounts {
    int n[BRIEF_MAXBATCH];
};

// ---- 1. integral image (B2, B3): integral_scan.hip.h ----

// ---- 2. key-point filter (B4, OURS-1) ----
// mask[i] = 1 for a key point that stays, iota[i] = i (the compaction carries it along as kept_index)
__global__ __launch_bounds__(256) void brief_flag_kernel(const float *__restrict__ xy_all, BriefCounts n_in, int cap, int w, int h,
                                                         uint8_t *__restrict__ mask_all, int mask_stride, int *__restrict__ iota_all)
{
    const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (i >= n_in.n[b])
        return;
    const float *__restrict__ src = xy_all + 2 * ((size_t)b * cap + i);   // the caller's array: 4-byte alignment is all it has
    const float2 p = make_float2(src[0], src[1]);
    bool keep = false;
    if (w > 2 * BRIEF_BORDER && h > 2 * BRIEF_BORDER) {
        // Rect(28, 28, w - 56, h - 56).contains(Point(cvRound(x), cvRound(y))): round half to even; NaN and infinities fail
        const double rx = rint((double)p.x), ry = rint((double)p.y);
        keep = rx >= BRIEF_BORDER && rx < w - BRIEF_BORDER && ry >= BRIEF_BORDER && ry < h - BRIEF_BORDER;
        // OURS-1: the centre the sampling uses, (int)(x + 0.5), must leave the +24 offset inside the table
        keep = keep && (double)p.x + 0.5 < (double)(w - BRIEF_BORDER) && (double)p.y + 0.5 < (double)(h - BRIEF_BORDER);
    }
    mask_all[(size_t)b * mask_stride + i] = keep ? 1 : 0;
    iota_all[(size_t)b * cap + i] = i;
}

// ---- 3. descriptors (B5, B6) ----
// the 9 x 9 box sum around (iy, ix): rows iy - 4 ... iy + 4, columns ix - 4 ... ix + 4
__device__ __forceinline__ int brief_smoothed(const int *__restrict__ sum, int pitch, int iy, int ix)
{
    const int *a = sum + (size_t)(iy - 4) * pitch + ix, *b = sum + (size_t)(iy + 5) * pitch + ix;
    return b[5] - b[-4] - a[5] + a[-4];
}

template <int ROUNDS>
__global__ __launch_bounds__(64 * BRIEF_WAVES) void brief_describe_kernel(const int *__restrict__ sum_all, long long img_stride, int w,
                                                                          const float *__restrict__ kxy_all, const int *__restrict__ d_count,
                                                                          int cap, const int8_t *__restrict__ table,
                                                                          uint8_t *__restrict__ desc_all)
{
    constexpr int BYTES = 8 * ROUNDS;
    __shared__ char4 tests[64 * ROUNDS];
    for (int t = threadIdx.x; t < 64 * ROUNDS; t += 64 * BRIEF_WAVES)
        tests[t] = reinterpret_cast<const char4 *>(table)[t];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.y;
    const int n = min(d_count[b], cap), pitch = w + 1;
    const int *__restrict__ sum = sum_all + b * img_stride;
    const float2 *__restrict__ kxy = reinterpret_cast<const float2 *>(kxy_all) + (size_t)b * cap;
    uint8_t *__restrict__ desc = desc_all + (size_t)b * cap * BYTES;
    for (int k = blockIdx.x * BRIEF_WAVES + wave; k < n; k += gridDim.x * BRIEF_WAVES) {
        const float2 p = kxy[k];
        const int cx = (int)((double)p.x + 0.5), cy = (int)((double)p.y + 0.5);
        unsigned long long word[ROUNDS];
#pragma unroll
        for (int r = 0; r < ROUNDS; r++) {
            const char4 t = tests[64 * r + lane];   // (y1, x1, y2, x2)
            const int s1 = brief_smoothed(sum, pitch, cy + (int)(signed char)t.x, cx + (int)(signed char)t.y);
            const int s2 = brief_smoothed(sum, pitch, cy + (int)(signed char)t.z, cx + (int)(signed char)t.w);
            word[r] = __ballot(s1 < s2);
        }
        // test 64 r + j sits at bit j of word r and belongs at bit 7 - j % 8 of byte 8 r + j / 8: lane l < BYTES takes byte l % 8 of
        // word l / 8 and turns it round
        if (lane < BYTES) {
            unsigned long long mine = word[0];
#pragma unroll
            for (int r = 1; r < ROUNDS; r++)
                mine = (lane >> 3) == r ? word[r] : mine;
            const unsigned byte = (unsigned)(mine >> (8 * (lane & 7))) & 0xffu;
            desc[(size_t)k * BYTES + lane] = (uint8_t)(__brev(byte) >> 24);
        }
    }
}

// ---- host side ----
int brief_slot(int bytes) { return bytes == 16 ? 0 : bytes == 32 ? 1 : bytes == 64 ? 2 : -1; }

const int8_t *brief_default(int slot) { return slot == 0 ? BRIEF_DEFAULT_16 : slot == 1 ? BRIEF_DEFAULT_32 : BRIEF_DEFAULT_64; }

int brief_check_image(int w, int h, int c)
{
    SVO_CHECK_ARG(c == 1 || c == 3);
    SVO_CHECK_ARG(w >= 1 && h >= 1 && w <= 16384 && h <= 16384);
    if (!integral_fits_int32(w, h)) {
        svo_set_error("svo_brief: the int32 integral image of %d x %d pixels could overflow (255 w h > 2^31 - 1)", w, h);
        return SVO_ERR_CAPACITY;
    }
    return SVO_OK;
}

// the current table of `slot` on the device
int brief_table(svo_ctx *ctx, int slot, const int8_t **d_table)
{
    int rc;
    if ((rc = ctx->brief_pat.ensure(3 * 2048)))
        return rc;
    int8_t *dst = ctx->brief_pat.as<int8_t>() + 2048 * slot;
    if (!ctx->brief_pat_live[slot]) {
        const int8_t *src = ctx->brief_has_pattern[slot] ? ctx->brief_pattern[slot] : brief_default(slot);
        SVO_HIP(hipMemcpyAsync(dst, src, (size_t)32 * (16 << slot), hipMemcpyHostToDevice, ctx->stream));
        SVO_HIP(hipStreamSynchronize(ctx->stream));   // the source may be replaced by the next svo_brief_set_pattern
        ctx->brief_pat_live[slot] = 1;
    }
    *d_table = dst;
    return SVO_OK;
}

// the integral images of nb device images into ctx->feat_sum
int brief_integrals(svo_ctx *ctx, const uint8_t *const *d_images, int nb, int w, int h, int c)
{
    ScopedKernelTime tm(ctx, SVO_K_BRIEF_INTEGRAL);
    return integral_images(ctx, d_images, nb, w, h, c, 0);
}

}  // namespace

extern "C" {

int svo_brief_default_pattern(int bytes, int8_t *pattern)
{
    const int slot = brief_slot(bytes);
    SVO_CHECK_ARG(slot >= 0 && pattern);
    memcpy(pattern, brief_default(slot), (size_t)32 * bytes);
    return SVO_OK;
}

int svo_brief_set_pattern(svo_ctx *ctx, int bytes, const int8_t *pattern)
{
    const int slot = brief_slot(bytes);
    SVO_CHECK_ARG(ctx && slot >= 0);
    if (pattern) {
        for (int t = 0; t < 8 * bytes; t++) {
            const int8_t *q = pattern + 4 * t;
            for (int k = 0; k < 4; k++)
                if (q[k] < -BRIEF_HALF_PATCH || q[k] > BRIEF_HALF_PATCH) {
                    svo_set_error("svo_brief_set_pattern: test %d has the offset %d (|.| <= 24: a sample must stay inside the 48-pixel "
                                  "patch)", t, (int)q[k]);
                    return SVO_ERR_ARG;
                }
            if (q[0] == q[2] && q[1] == q[3]) {
                svo_set_error("svo_brief_set_pattern: the end points of test %d are equal", t);
                return SVO_ERR_ARG;
            }
        }
        memcpy(ctx->brief_pattern[slot], pattern, (size_t)32 * bytes);
        ctx->brief_has_pattern[slot] = 1;
    } else {
        ctx->brief_has_pattern[slot] = 0;
    }
    ctx->brief_pat_live[slot] = 0;
    return SVO_OK;
}

int svo_brief_integral(svo_ctx *ctx, const uint8_t *image, int w, int h, int c, int32_t *sum, int mem)
{
    SVO_CHECK_ARG(ctx && image && sum && aligned4(sum));
    SVO_CHECK_ARG(mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE);
    int rc;
    if ((rc = brief_check_image(w, h, c)))
        return rc;
    SVO_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint8_t *d_img = nullptr;
    if ((rc = stage_images(ctx, &image, 1, (size_t)w * h * c, mem, &d_img)) || (rc = brief_integrals(ctx, &d_img, 1, w, h, c)))
        return rc;
    SVO_HIP(hipMemcpyAsync(sum, ctx->feat_sum.p, (size_t)(w + 1) * (h + 1) * 4,
                           mem == SVO_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, st));
    if (mem == SVO_MEM_HOST)
        SVO_HIP(hipStreamSynchronize(st));
    return SVO_OK;
}

int svo_brief_describe_batch(svo_ctx *ctx, const uint8_t *const *images, int n_images, int w, int h, int c, int bytes, const float *xy,
                             const int *n_in, int cap, int *kept_index, uint8_t *desc, int *n_out, int mem)
{
    SVO_CHECK_ARG(ctx && images && xy && n_in && kept_index && desc && n_out);
    SVO_CHECK_ARG(mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE);
    SVO_CHECK_ARG(aligned4(xy) && aligned4(n_in) && aligned4(kept_index) && aligned4(n_out));
    SVO_CHECK_ARG(n_images >= 1 && n_images <= BRIEF_MAXBATCH && cap >= 1);
    const int slot = brief_slot(bytes);
    SVO_CHECK_ARG(slot >= 0);
    int n_max = 0;
    for (int k = 0; k < n_images; k++) {
        SVO_CHECK_ARG(images[k] != nullptr);
        SVO_CHECK_ARG(n_in[k] >= 0 && n_in[k] <= cap);
        n_max = n_in[k] > n_max ? n_in[k] : n_max;
    }
    int rc;
    if ((rc = brief_check_image(w, h, c)))
        return rc;
    if (w <= 2 * BRIEF_BORDER || h <= 2 * BRIEF_BORDER || n_max == 0) {   // runByImageBorder removes every key point
        for (int k = 0; k < n_images; k++)
            n_out[k] = 0;
        return SVO_OK;
    }
    SVO_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int8_t *d_table = nullptr;
    if ((rc = brief_table(ctx, slot, &d_table)))
        return rc;
    const size_t e = (size_t)n_images * cap;
    const int mask_stride = (cap + 15) & ~15;
    const bool host = mem == SVO_MEM_HOST;
    if ((rc = ctx->brief_work.ensure(e * (8 + 4 + 8 + (host ? 4 + (size_t)bytes : 0)) + (size_t)n_images * mask_stride + 8 * 256 + 256)))
        return rc;
    uint8_t *q = ctx->brief_work.as<uint8_t>();
    int *d_counts = bump<int>(q, BRIEF_MAXBATCH);
    uint8_t *d_mask = bump<uint8_t>(q, (size_t)n_images * mask_stride);
    int *d_iota = bump<int>(q, e);
    float *d_kxy = bump<float>(q, 2 * e);
    const float *d_xy = xy;
    int *d_kept = kept_index;
    uint8_t *d_desc = desc;
    const uint8_t *ptrs[BRIEF_MAXBATCH];
    if (host) {
        float *sxy = bump<float>(q, 2 * e);
        d_kept = bump<int>(q, e);
        d_desc = bump<uint8_t>(q, e * bytes);
        for (int k = 0; k < n_images; k++)
            if (n_in[k])
                SVO_HIP(hipMemcpyAsync(sxy + 2 * (size_t)k * cap, xy + 2 * (size_t)k * cap, (size_t)n_in[k] * 8, hipMemcpyHostToDevice, st));
        d_xy = sxy;
    }
    if ((rc = stage_images(ctx, images, n_images, (size_t)w * h * c, mem, ptrs)) || (rc = brief_integrals(ctx, ptrs, n_images, w, h, c)))
        return rc;
    {
        ScopedKernelTime tm(ctx, SVO_K_BRIEF_DESCRIBE);
        BriefCounts cnt;
        for (int k = 0; k < BRIEF_MAXBATCH; k++)
            cnt.n[k] = k < n_images ? n_in[k] : 0;
        hipLaunchKernelGGL(brief_flag_kernel, dim3((n_max + 255) / 256, n_images), dim3(256), 0, st, d_xy, cnt, cap, w, h, d_mask,
                           mask_stride, d_iota);
        svo_compact_job jobs[BRIEF_MAXBATCH];
        for (int k = 0; k < n_images; k++) {
            svo_compact_job &j = jobs[k];
            j.mask = d_mask + (size_t)k * mask_stride;
            j.cap = n_in[k];
            j.d_n = nullptr;
            j.in[0] = d_xy + 2 * (size_t)k * cap;
            j.out[0] = d_kxy + 2 * (size_t)k * cap;
            j.stride[0] = 2;
            j.in[1] = reinterpret_cast<const float *>(d_iota + (size_t)k * cap);   // moved as 32-bit words
            j.out[1] = reinterpret_cast<float *>(d_kept + (size_t)k * cap);
            j.stride[1] = 1;
            j.in[2] = nullptr;
            j.out[2] = nullptr;
            j.stride[2] = 0;
            j.d_count = d_counts + k;
        }
        if ((rc = svo_launch_compact_batch(ctx, n_images, jobs)))
            return rc;
        int gx = (n_max + BRIEF_WAVES - 1) / BRIEF_WAVES;
        gx = gx > BRIEF_MAXGRID ? BRIEF_MAXGRID : gx;
        const dim3 grid(gx, n_images), block(64 * BRIEF_WAVES);
        const int *sums = ctx->feat_sum.as<int>();
        const long long stride = integral_img_stride(w, h);
        if (slot == 0)
            hipLaunchKernelGGL(brief_describe_kernel<2>, grid, block, 0, st, sums, stride, w, d_kxy, d_counts, cap, d_table, d_desc);
        else if (slot == 1)
            hipLaunchKernelGGL(brief_describe_kernel<4>, grid, block, 0, st, sums, stride, w, d_kxy, d_counts, cap, d_table, d_desc);
        else
            hipLaunchKernelGGL(brief_describe_kernel<8>, grid, block, 0, st, sums, stride, w, d_kxy, d_counts, cap, d_table, d_desc);
        SVO_HIP(hipGetLastError());
    }
    // the one wait: the counts
    if ((rc = read_counts(ctx, d_counts, n_images, n_out)))
        return rc;
    if (host) {
        const HostColumn cols[2] = {{kept_index, d_kept, 4}, {desc, d_desc, (size_t)bytes}};
        return copy_rows_to_host(st, cols, 2, n_images, cap, n_out);
    }
    return SVO_OK;
}

}  // extern "C"
