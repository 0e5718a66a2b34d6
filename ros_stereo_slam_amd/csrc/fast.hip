// fast.hip -- cv::FAST (TYPE_9_16) as a detector of its own, and the FAST -> ANMS key-point source, for gfx950.
//
// Replaces cv::FAST(image, kps, threshold, nonmaxSuppression) as the demo around adaptiveNonMaximalSuppresion calls it
// (src/ANMS.cpp:69-82).  The definition is the one tests/fast_numpy.py states: the segment test on the
// radius-3 ring, the corner score = the largest threshold at which the pixel still fires, 3 x 3 suppression with strict
// comparisons, key points in row-major order, KeyPointsFilter::retainBest with ties.
//
// Launches of one call, the image index on a grid axis (up to 16 images of one size):
//   fast_grey_kernel      BGR -> grey with cvtColor's integer weights (or a copy of a grey image whose rows are not whole dwords)
//                         into a plane with a 4-byte pitch, so that the score launch stages tiles with dword loads
//   fast_score_kernel     a 64 x 16 tile and its halo in LDS, the pre-test on opposite ring pixels, the segment test, the score of the
//                         pixels that fire; writes the `fired` plane (0 = no corner, else score + 1: a corner at threshold 0 may
//                         score 0) and, when asked for, the public score plane
//   fast_compact_kernel   <false>: a wavefront counts the key points among its 1024 consecutive pixels of the row-major plane (ballot +
//                         popcount) and, for retainBest, adds their scores to the image's 256-bin histogram
//   fast_scan_kernel      one workgroup per image: exclusive scan of the wavefronts' counts (scan_ops.hip.h), the total, the cut of
//                         retainBest
//   fast_compact_kernel   <true>: the same walk again, each key point written at offset + rank inside the wavefront
// No atomic decides a position: the order of the output is the order of the pixels.  With retainBest the count / scan pair runs a
// second time with the cut applied.  The chained call hands the lists to anms.hip's launches without leaving the device.
#include "svo_internal.h"

#include "fast_plan.hip.h"
#include "scan_ops.hip.h"

namespace {

#include "feature_batch.hip.h"

using namespace fast_plan;
static_assert(MAX_BATCH == IMAGE_MAXBATCH, "one image table for every batched entry point");
static_assert(TILE_W == 64 && TILE_H % 4 == 0 && LDS_PITCH % 4 == 0, "a wavefront spans a tile row; the workgroup's four wavefronts step four rows");

// ---------------------------------------------------------------------------------------------------------------- grey plane
// one lane per dword of the pitched plane; the bytes past column w - 1 are zero
__global__ __launch_bounds__(256) void fast_grey_kernel(ImageBatch src, int w, int h, int c, int pitch, uint8_t *grey, size_t plane_bytes)
{
    const int dwords = pitch >> 2;
    const unsigned i = blockIdx.x * 256u + threadIdx.x;   // < 2^26
    if (i >= (unsigned)dwords * (unsigned)h)
        return;
    const int y = i / dwords, x4 = (i - y * dwords) * 4;
    const uint8_t *__restrict__ s = src.img[blockIdx.y];
    uint32_t out = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int x = x4 + j;
        if (x < w) {
            const size_t p = (size_t)y * w + x;
            const int g = c == 1 ? s[p] : svo_bgr2gray(s[3 * p], s[3 * p + 1], s[3 * p + 2]);
            out |= (uint32_t)g << (8 * j);
        }
    }
    reinterpret_cast<uint32_t *>(grey + blockIdx.y * plane_bytes)[i] = out;
}

// ---------------------------------------------------------------------------------------------------------------- score
// offsets of the ring in the staged tile: clockwise from twelve o'clock (tests/orb_numpy.py: RING)
__device__ __forceinline__ constexpr int ring_off(int k)
{
    constexpr int dx[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
    constexpr int dy[16] = {-3, -3, -2, -1, 0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3};
    return dy[k] * LDS_PITCH + dx[k];
}

// nine cyclically contiguous bits among the 16 of m
__device__ __forceinline__ bool arc9(unsigned m)
{
    unsigned x = m | (m << 16);
    x &= x >> 1;
    x &= x >> 2;
    x &= x >> 4;   // runs of 8
    x &= x >> 1;   // runs of 9
    return (x & 0xffffu) != 0;
}

// 0 when the pixel does not fire at t, else its score + 1 (1 ... 255)
__device__ __forceinline__ int fast_pixel(const uint8_t *__restrict__ p, int t)
{
    const int c = p[0], lo = c - t, hi = c + t;
    // bit 0: darker, bit 1: brighter.  An arc of nine holds one of every two opposite ring pixels.
    auto cls = [&](int k) { const int v = p[ring_off(k)]; return (v < lo ? 1 : 0) | (v > hi ? 2 : 0); };
    int d = cls(0) | cls(8);
    if (!d)
        return 0;
    d &= cls(4) | cls(12);
    if (!d)
        return 0;
    d &= cls(2) | cls(10);
    d &= cls(6) | cls(14);
    if (!d)
        return 0;
    int v[16];
    unsigned bright = 0, dark = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        v[k] = (int)p[ring_off(k)] - c;
        bright |= (v[k] > t ? 1u : 0u) << k;
        dark |= (v[k] < -t ? 1u : 0u) << k;
    }
    if (!arc9(bright) && !arc9(dark))
        return 0;
    // min and max over every arc of nine by doubling: 2, 4, 8 and one more
    int mn[16], mx[16], a[16], b[16];
#pragma unroll
    for (int k = 0; k < 16; k++) {
        a[k] = min(v[k], v[(k + 1) & 15]);
        b[k] = max(v[k], v[(k + 1) & 15]);
    }
#pragma unroll
    for (int k = 0; k < 16; k++) {
        mn[k] = min(a[k], a[(k + 2) & 15]);
        mx[k] = max(b[k], b[(k + 2) & 15]);
    }
#pragma unroll
    for (int k = 0; k < 16; k++) {
        a[k] = min(mn[k], mn[(k + 4) & 15]);
        b[k] = max(mx[k], mx[(k + 4) & 15]);
    }
    int best = -256;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        best = max(best, min(a[k], v[(k + 8) & 15]));
        best = max(best, -max(b[k], v[(k + 8) & 15]));
    }
    return best;   // (best - 1) + 1; best > t >= 0 here
}

__global__ __launch_bounds__(256) void fast_score_kernel(ImageBatch src, int pitch, int w, int h, int t, uint8_t *fired,
                                                         size_t plane_bytes, uint8_t *score)
{
    __shared__ uint32_t tile[LDS_ROWS * LDS_DWORDS];
    const int x0 = blockIdx.x * TILE_W, y0 = blockIdx.y * TILE_H;
    const uint8_t *__restrict__ s = src.img[blockIdx.z];
    for (int i = threadIdx.x; i < LDS_ROWS * LDS_DWORDS; i += 256) {
        const int r = i / LDS_DWORDS, d = i - r * LDS_DWORDS;
        const int gy = y0 - BORDER + r, gx = x0 - 4 + 4 * d;
        uint32_t v = 0;
        if (gy >= 0 && gy < h && gx >= 0 && gx + 4 <= pitch)
            v = *reinterpret_cast<const uint32_t *>(s + (size_t)gy * pitch + gx);
        tile[i] = v;
    }
    __syncthreads();
    const uint8_t *tb = reinterpret_cast<const uint8_t *>(tile);
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int x = x0 + tx;
    if (x >= w)
        return;
    uint8_t *__restrict__ f = fired + blockIdx.z * plane_bytes;
    uint8_t *__restrict__ sc = score ? score + blockIdx.z * ((size_t)w * h) : nullptr;
#pragma unroll
    for (int k = 0; k < TILE_H / 4; k++) {
        const int ly = ty + 4 * k, y = y0 + ly;
        if (y >= h)
            break;
        int v = 0;
        if (x >= BORDER && x < w - BORDER && y >= BORDER && y < h - BORDER)
            v = fast_pixel(tb + (ly + BORDER) * LDS_PITCH + tx + 4, t);
        f[(size_t)y * pitch + x] = (uint8_t)v;
        if (sc)
            sc[(size_t)y * w + x] = (uint8_t)(v ? v - 1 : 0);
    }
}

// ---------------------------------------------------------------------------------------------------------------- compaction
// 0, or the fired value (score + 1) of a key point.  Suppression: the score strictly above the eight neighbours' (0 where they do not
// fire), i.e. fired >= 2 and above every neighbour's fired value; `cut` is retainBest's.
__device__ __forceinline__ int fast_keep(const uint8_t *__restrict__ f, int pitch, int x, int y, int nonmax, int cut)
{
    const uint8_t *q = f + (size_t)y * pitch + x;
    const int v = q[0];
    if (!v || !nonmax)
        return v;
    // a pixel that fires is at least 3 inside: its neighbours are in the plane
    if (v < 2 || v - 1 < cut)
        return 0;
    const int m = max(max(max(q[-pitch - 1], q[-pitch]), max(q[-pitch + 1], q[-1])),
                      max(max(q[1], q[pitch - 1]), max(q[pitch], q[pitch + 1])));
    return v > m ? v : 0;
}

template <bool SCATTER>
__global__ __launch_bounds__(64 * WAVES) void fast_compact_kernel(const uint8_t *fired, size_t plane_bytes, int pitch, int w, int h, int nonmax,
                                                                 const int *cut, int spans, int *span_count, int *hist,
                                                                 const int *span_offset, int cap, size_t list_stride, float *xy, float *resp)
{
    __shared__ int s_hist[256];
    const int img = blockIdx.y, lane = threadIdx.x & 63;
    const int span = blockIdx.x * WAVES + (threadIdx.x >> 6);
    const bool live = span < spans;   // wave-uniform
    const uint8_t *__restrict__ f = fired + img * plane_bytes;
    const int c = cut ? cut[img] : 0;
    const unsigned npix = (unsigned)w * (unsigned)h;   // <= 2^28
    if (!SCATTER && hist) {   // kernel-uniform
        s_hist[threadIdx.x] = 0;
        __syncthreads();
    }
    int base = 0;
    if (live) {
        if (SCATTER)
            base = span_offset[(size_t)img * spans + span];
        float2 *__restrict__ oxy = reinterpret_cast<float2 *>(xy) + img * list_stride;
        float *__restrict__ orp = resp ? resp + img * list_stride : nullptr;
        for (int i = 0; i < SPAN / 64; i++) {
            const unsigned idx = (unsigned)span * SPAN + i * 64 + lane;
            int v = 0, x = 0, y = 0;
            if (idx < npix) {
                y = idx / (unsigned)w;
                x = idx - (unsigned)y * w;
                v = fast_keep(f, pitch, x, y, nonmax, c);
            }
            const unsigned long long m = __ballot(v != 0);
            if (SCATTER) {
                const int pos = base + svo::lanes_below(m);
                if (v && pos < cap) {
                    oxy[pos] = make_float2((float)x, (float)y);
                    if (orp)
                        orp[pos] = nonmax ? (float)(v - 1) : 0.f;
                }
            } else if (hist && v) {
                atomicAdd(&s_hist[v - 1], 1);   // counts only: no order depends on it
            }
            base += __popcll(m);
        }
        if (!SCATTER && lane == 0)
            span_count[(size_t)img * spans + span] = base;
    }
    if (!SCATTER && hist) {
        __syncthreads();
        const int k = s_hist[threadIdx.x];
        if (k)
            atomicAdd(&hist[img * 256 + threadIdx.x], k);
    }
}

// one workgroup per image: span_offset = exclusive scan of span_count, counts[img] = the total, cut[img] from the histogram
__global__ __launch_bounds__(256) void fast_scan_kernel(const int *span_count, int *span_offset, int spans, int *counts, const int *hist,
                                                        int max_keypoints, int *cut)
{
    __shared__ int s_wave[4];
    const int img = blockIdx.x;
    const int total = svo::block_scan_counts<256>(span_count + (size_t)img * spans, span_offset + (size_t)img * spans, spans, s_wave);
    if (threadIdx.x == 0) {
        counts[img] = total;
        if (hist)
            cut[img] = retain_cut(hist + img * 256, max_keypoints);
    }
}

// the chained call's last step: out[j] = in[idx[j]] for the *count key points ANMS kept
__global__ __launch_bounds__(256) void fast_gather_kernel(const float2 *xy, const float *resp, const int *idx, const int *count, float2 *oxy,
                                                          float *oresp)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= *count)
        return;
    const int i = idx[j];
    oxy[j] = xy[i];
    if (oresp)
        oresp[j] = resp[i];
}

// the first min(n[k], cap) rows of every list to the caller's host arrays (cap rows apart there, `stride` rows apart on the device), then
// the wait for them
int copy_lists(hipStream_t st, const HostColumn *cols, int n_images, int cap, size_t stride, const int *n)
{
    for (int k = 0; k < n_images; k++) {
        const size_t m = (size_t)(n[k] < cap ? n[k] : cap);
        if (!m)
            continue;
        for (int c = 0; c < 2; c++)
            if (cols[c].host)
                SVO_HIP(hipMemcpyAsync(static_cast<uint8_t *>(cols[c].host) + (size_t)k * cap * cols[c].bytes,
                                       static_cast<const uint8_t *>(cols[c].dev) + k * stride * cols[c].bytes, m * cols[c].bytes,
                                       hipMemcpyDeviceToHost, st));
    }
    SVO_HIP(hipStreamSynchronize(st));
    return SVO_OK;
}

int fast_refuse(const char *fn, const char *why)
{
    svo_set_error("%s: %s", fn, why);
    return SVO_ERR_ARG;
}

// both entry points.  keep < 0: detection alone.
int fast_run(const char *fn, svo_ctx *ctx, const uint8_t *const *images, int n_images, int w, int h, int c, const svo_fast_params *prm,
             int keep, int cap, float *xy, float *response, uint8_t *score, int *n, int mem)
{
    const bool anms = keep >= 0;
    if (!ctx)
        return fast_refuse(fn, "ctx must not be null");
    if (const char *why = check_args(images, prm, xy, n, n_images, w, h, c, cap))
        return fast_refuse(fn, why);
    if (mem != SVO_MEM_HOST && mem != SVO_MEM_DEVICE)
        return fast_refuse(fn, "mem must be SVO_MEM_HOST or SVO_MEM_DEVICE");
    if (anms && keep < 1)
        return fast_refuse(fn, "num_to_keep must be at least 1");
    if (!aligned4(xy) || !aligned4(response) || !aligned4(n))
        return fast_refuse(fn, "xy, response and n must be 4-byte aligned");
    for (int k = 0; k < n_images; k++)
        if (!images[k])
            return fast_refuse(fn, "an image pointer is null");
    const bool host = mem == SVO_MEM_HOST;
    SVO_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t px = (size_t)w * h;
    if (w < 2 * BORDER + 1 || h < 2 * BORDER + 1) {   // no pixel has its ring inside the image
        for (int k = 0; k < n_images; k++)
            n[k] = 0;
        if (score && host)
            memset(score, 0, px * n_images);
        else if (score)
            SVO_HIP(hipMemsetAsync(score, 0, px * n_images, st));
        return SVO_OK;
    }
    // a grey image whose rows are whole dwords at a dword address is read where it is
    const uint8_t *ptrs[MAX_BATCH];
    int rc;
    if ((rc = stage_images(ctx, images, n_images, px * c, mem, ptrs)))
        return rc;
    bool in_place = c == 1 && (w & 3) == 0;
    for (int k = 0; k < n_images; k++)
        in_place = in_place && aligned4(ptrs[k]);
    const size_t lcap = (size_t)cap < px ? (size_t)cap : px;   // no image has more key points than pixels
    const Plan p = make_plan(w, h, c, n_images, (int)lcap, !in_place, host && score, host, anms);
    if ((rc = ctx->fast_work.ensure(p.total)))
        return rc;
    uint8_t *wb = ctx->fast_work.as<uint8_t>();
    auto at = [wb](size_t off) { return wb + off; };
    int *d_counts = reinterpret_cast<int *>(at(p.off_counts)), *d_hist = reinterpret_cast<int *>(at(p.off_hist));
    int *d_cut = reinterpret_cast<int *>(at(p.off_cut));
    int *d_span_count = reinterpret_cast<int *>(at(p.off_span_count)), *d_span_offset = reinterpret_cast<int *>(at(p.off_span_offset));
    uint8_t *d_fired = at(p.off_fired);
    const bool own_lists = host || anms;
    float *d_xy = own_lists ? reinterpret_cast<float *>(at(p.off_xy)) : xy;
    float *d_resp = own_lists ? reinterpret_cast<float *>(at(p.off_resp)) : response;
    const size_t stride = own_lists ? lcap : (size_t)cap;
    uint8_t *d_score = !score ? nullptr : host ? at(p.off_score) : score;

    ImageBatch grey = make_image_batch(ptrs, n_images);
    if (!in_place) {
        const unsigned dw = (unsigned)(p.pitch >> 2) * (unsigned)h;
        hipLaunchKernelGGL(fast_grey_kernel, dim3((dw + 255) / 256, n_images), dim3(256), 0, st, grey, w, h, c, p.pitch, at(p.off_grey),
                           p.plane_bytes);
        for (int k = 0; k < n_images; k++)
            grey.img[k] = at(p.off_grey) + k * p.plane_bytes;
    }
    hipLaunchKernelGGL(fast_score_kernel, dim3(p.tiles_x, p.tiles_y, n_images), dim3(256), 0, st, grey, p.pitch, w, h, prm->threshold,
                       d_fired, p.plane_bytes, d_score);
    const int nonmax = prm->nonmax_suppression != 0;
    // without suppression every response is 0: retainBest's cut is 0 and everything stays
    const bool retain = nonmax && prm->max_keypoints > 0;
    const dim3 cgrid(p.groups, n_images), cblock(64 * WAVES);
    if (retain)
        SVO_HIP(hipMemsetAsync(d_hist, 0, sizeof(int) * 256 * n_images, st));
    hipLaunchKernelGGL(fast_compact_kernel<false>, cgrid, cblock, 0, st, d_fired, p.plane_bytes, p.pitch, w, h, nonmax, (const int *)nullptr,
                       p.spans, d_span_count, retain ? d_hist : nullptr, (const int *)nullptr, 0, stride, (float *)nullptr, (float *)nullptr);
    hipLaunchKernelGGL(fast_scan_kernel, dim3(n_images), dim3(256), 0, st, d_span_count, d_span_offset, p.spans, d_counts,
                       retain ? d_hist : nullptr, prm->max_keypoints, d_cut);
    if (retain) {
        hipLaunchKernelGGL(fast_compact_kernel<false>, cgrid, cblock, 0, st, d_fired, p.plane_bytes, p.pitch, w, h, nonmax, d_cut, p.spans,
                           d_span_count, (int *)nullptr, (const int *)nullptr, 0, stride, (float *)nullptr, (float *)nullptr);
        hipLaunchKernelGGL(fast_scan_kernel, dim3(n_images), dim3(256), 0, st, d_span_count, d_span_offset, p.spans, d_counts,
                           (const int *)nullptr, 0, d_cut);
    }
    const int wcap = (int)(stride < (size_t)cap ? stride : (size_t)cap);
    hipLaunchKernelGGL(fast_compact_kernel<true>, cgrid, cblock, 0, st, d_fired, p.plane_bytes, p.pitch, w, h, nonmax,
                       retain ? d_cut : (const int *)nullptr, p.spans, d_span_count, (int *)nullptr, d_span_offset, wcap, stride, d_xy,
                       anms || response ? d_resp : (float *)nullptr);
    SVO_HIP(hipGetLastError());
    // the one wait of a detection: the counts, through pinned memory
    int *pin = reinterpret_cast<int *>(ctx->pinned);
    SVO_HIP(hipMemcpyAsync(pin, d_counts, sizeof(int) * n_images, hipMemcpyDeviceToHost, st));
    SVO_HIP(hipStreamSynchronize(st));
    bool over = false;
    for (int k = 0; k < n_images; k++) {
        n[k] = pin[k];
        over = over || n[k] > cap;
    }
    if (host && score)
        SVO_HIP(hipMemcpyAsync(score, d_score, px * n_images, hipMemcpyDeviceToHost, st));
    if (over) {
        if (host && !anms) {
            const HostColumn cols[2] = {{xy, d_xy, 8}, {response, d_resp, 4}};
            if ((rc = copy_lists(st, cols, n_images, cap, stride, n)))
                return rc;
        }
        svo_set_error("%s: an image has more than cap = %d key points (n[] holds the counts)", fn, cap);
        return SVO_ERR_CAPACITY;
    }
    if (!anms) {
        if (host) {
            const HostColumn cols[2] = {{xy, d_xy, 8}, {response, d_resp, 4}};
            return copy_lists(st, cols, n_images, cap, stride, n);
        }
        return SVO_OK;
    }
    // FAST -> ANMS: the lists stay where they are, anms.hip's launches rank them image by image (its scratch is the context's w_a,
    // w_b, w_d; one stream orders the images), the kept key points are gathered in ANMS's order
    int *d_idx = reinterpret_cast<int *>(at(p.off_idx)), *d_kept = reinterpret_cast<int *>(at(p.off_kept));
    float *o_xy = host ? reinterpret_cast<float *>(at(p.off_oxy)) : xy;
    float *o_resp = host ? reinterpret_cast<float *>(at(p.off_oresp)) : response;
    const size_t ostride = host ? stride : (size_t)cap;
    SVO_HIP(hipMemsetAsync(d_kept, 0, sizeof(int) * MAX_BATCH, st));
    for (int k = 0; k < n_images; k++) {
        if (!n[k])
            continue;
        const float *kxy = d_xy + 2 * stride * k, *krp = d_resp + stride * k;
        if ((rc = svo_launch_anms(ctx, kxy, krp, n[k], keep, d_idx + stride * k, d_kept + k)))
            return rc;
        hipLaunchKernelGGL(fast_gather_kernel, dim3((n[k] + 255) / 256), dim3(256), 0, st, reinterpret_cast<const float2 *>(kxy), krp,
                           d_idx + stride * k, d_kept + k, reinterpret_cast<float2 *>(o_xy) + ostride * k,
                           response ? o_resp + ostride * k : (float *)nullptr);
    }
    SVO_HIP(hipGetLastError());
    SVO_HIP(hipMemcpyAsync(pin, d_kept, sizeof(int) * n_images, hipMemcpyDeviceToHost, st));
    SVO_HIP(hipStreamSynchronize(st));
    for (int k = 0; k < n_images; k++)
        n[k] = pin[k];
    if (host) {
        const HostColumn cols[2] = {{xy, o_xy, 8}, {response, o_resp, 4}};
        return copy_lists(st, cols, n_images, cap, ostride, n);
    }
    return SVO_OK;
}

}  // namespace

extern "C" {

void svo_fast_default_params(svo_fast_params *p)
{
    if (!p)
        return;
    p->threshold = 10;
    p->nonmax_suppression = 1;
    p->max_keypoints = 0;
}

int svo_fast_detect_batch(svo_ctx *ctx, const uint8_t *const *images, int n_images, int w, int h, int c, const svo_fast_params *prm,
                          int cap, float *xy, float *response, uint8_t *score, int *n, int mem)
{
    return fast_run("svo_fast_detect_batch", ctx, images, n_images, w, h, c, prm, -1, cap, xy, response, score, n, mem);
}

int svo_fast_anms_batch(svo_ctx *ctx, const uint8_t *const *images, int n_images, int w, int h, int c, const svo_fast_params *prm,
                        int num_to_keep, int cap, float *xy, float *response, int *n, int mem)
{
    return fast_run("svo_fast_anms_batch", ctx, images, n_images, w, h, c, prm, num_to_keep < 0 ? 0 : num_to_keep, cap, xy, response,
                    nullptr, n, mem);
}

}  // extern "C"
