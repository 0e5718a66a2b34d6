// star.hip -- OpenCV 3.2's xfeatures2d::StarDetector (CenSurE), the detector of the commented Star + BRIEF pair above
// visualSLAM::stereoTriangulate (src/triangulation.cpp:79-80), for gfx950.
//
// The algorithm is stated operation by operation in tests/star_numpy.py (points S1 ... S7 as recalled from upstream, OURS-1 where
// upstream would read past its tables) and DESIGN.md section 10m.  Everything up to the star sums is int32 and exact; the float
// steps keep the stated operation order (the build's -ffp-contract=off keeps them apart).
//
// Launches of one call, the image index on a grid axis (up to 16 images of one size), all on the context's stream:
//   integral_row_scan / integral_col_scan   the upright table (integral_scan.hip.h)
//   star_diag_left_kernel                   a lane per diagonal x - y: the running sum down-right, into both cone tables
//   star_diag_right_kernel                  a lane per diagonal x + y: the running sum down-left, added to both cone tables
//   star_col_scan_kernel                    both cone tables added up along the columns.  even(x, y) = grey over y' <= y,
//                                           |x' - x| <= y - y'; odd(x, y) = grey over y' <= y, x - k <= x' <= x + 1 + k, k = y - y':
//                                           a diamond is even - odd - odd + even, four reads, as a square is of the upright table
//   star_response_kernel                    a lane per pixel: the star sums the patterns in use need, then the patterns
//   star_tile_kernel                        a lane per suppression tile: extrema, neighbourhood, size and line tests; a word per
//                                           tile, and the wavefront's key-point count (ballot + popcount)
//   star_scan_kernel                        one workgroup per image: exclusive scan of the wavefronts' counts (scan_ops.hip.h),
//                                           the total
//   star_scatter_kernel                     the tiles again: each key point written at offset + rank inside the wavefront
// No atomic decides a position: the order of the output is the order of the tiles.
#include <utility>

#include "svo_internal.h"

#include "scan_ops.hip.h"
#include "star_plan.hip.h"

namespace {

#include "feature_batch.hip.h"
#include "integral_scan.hip.h"

using namespace star_plan;
static_assert(MAX_BATCH == IMAGE_MAXBATCH, "one image table for every batched entry point");

__device__ __forceinline__ int star_grey(const uint8_t *__restrict__ s, int w, int c, int x, int y)
{
    const size_t p = (size_t)y * w + x;
    return c == 1 ? (int)s[p] : svo_bgr2gray(s[3 * p], s[3 * p + 1], s[3 * p + 2]);
}

// ---------------------------------------------------------------------------------------------------------------- cone tables
// Both tables are (h + 1) x (w + 1) like the upright one: entry [y + 1][x + 1] belongs to the apex (x, y), x = -1 ... w - 1; row 0
// (y = -1) is zero.  Lane d + h walks the diagonal x - y = d from y = -1 down: every entry of both tables is written once.
__global__ __launch_bounds__(256) void star_diag_left_kernel(ImageBatch im, int w, int h, int c, int *__restrict__ even_all,
                                                             int *__restrict__ odd_all, size_t stride)
{
    const int d = (int)(blockIdx.x * 256 + threadIdx.x) - h;
    if (d > w)
        return;
    const uint8_t *__restrict__ s = im.img[blockIdx.y];
    const size_t pitch = (size_t)w + 1;
    int *__restrict__ ev = even_all + blockIdx.y * stride, *__restrict__ od = odd_all + blockIdx.y * stride;
    int run = 0;
    // rows where -1 <= d + y <= w - 1
    const int ya = max(-1, -1 - d), yb = min(h - 1, w - 1 - d);
    for (int y0 = ya; y0 <= yb; y0 += 8) {
        int v[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int y = y0 + k, x = d + y;
            v[k] = y <= yb && y >= 0 && x >= 0 ? star_grey(s, w, c, x, y) : 0;
        }
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int y = y0 + k, x = d + y;
            if (y <= yb) {
                run += v[k];
                const size_t at = (size_t)(y + 1) * pitch + (x + 1);
                ev[at] = run;
                od[at] = run;
            }
        }
    }
}

// lane s + 1 walks the diagonal x + y = s, s = -1 ... w + h - 2, from y = 0 down: with R the running sum at (x, y),
// even(x, y) += R - grey(x, y) and odd(x - 1, y) += R; each entry is touched by one lane
__global__ __launch_bounds__(256) void star_diag_right_kernel(ImageBatch im, int w, int h, int c, int *__restrict__ even_all,
                                                              int *__restrict__ odd_all, size_t stride)
{
    const int sdiag = (int)(blockIdx.x * 256 + threadIdx.x) - 1;
    if (sdiag > w + h - 2)
        return;
    const uint8_t *__restrict__ s = im.img[blockIdx.y];
    const size_t pitch = (size_t)w + 1;
    int *__restrict__ ev = even_all + blockIdx.y * stride, *__restrict__ od = odd_all + blockIdx.y * stride;
    int run = 0;
    // rows where -1 <= s - y <= w - 1
    const int ya = max(0, sdiag - (w - 1)), yb = min(h - 1, sdiag + 1);
    for (int y0 = ya; y0 <= yb; y0 += 8) {
        int v[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int y = y0 + k, x = sdiag - y;
            v[k] = y <= yb && x >= 0 ? star_grey(s, w, c, x, y) : 0;
        }
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int y = y0 + k, x = sdiag - y;
            if (y <= yb) {
                run += v[k];
                const size_t at = (size_t)(y + 1) * pitch + (x + 1);
                ev[at] += run - v[k];
                if (x >= 0)
                    od[at - 1] += run;
            }
        }
    }
}

// a lane per column 0 ... w of one cone table (blockIdx.z: even, odd): rows 1 ... h added up from the top
__global__ __launch_bounds__(64) void star_col_scan_kernel(int w, int h, int *__restrict__ even_all, int *__restrict__ odd_all, size_t stride)
{
    const int x = blockIdx.x * 64 + threadIdx.x;
    if (x > w)
        return;
    const size_t pitch = (size_t)w + 1;
    int *__restrict__ p = (blockIdx.z ? odd_all : even_all) + blockIdx.y * stride + pitch + x;
    int acc = 0, y = 0;
    for (; y + 8 <= h; y += 8) {
        int v[8];
#pragma unroll
        for (int k = 0; k < 8; k++)
            v[k] = p[(size_t)(y + k) * pitch];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            acc += v[k];
            p[(size_t)(y + k) * pitch] = acc;
        }
    }
    for (; y < h; y++) {
        acc += p[(size_t)y * pitch];
        p[(size_t)y * pitch] = acc;
    }
}

// ---------------------------------------------------------------------------------------------------------------- responses
// the star sum of size index I at the pixel whose table entries up[y][x], ev[y][x], od[y][x] the pointers name
template <int I> __device__ __forceinline__ int star_sum(const int *__restrict__ up, const int *__restrict__ ev, const int *__restrict__ od, int pitch)
{
    constexpr int r = SIZES0[I], t = tilt(I);
    const int square = up[(r + 1) * pitch + r + 1] - up[-r * pitch + r + 1] - up[(r + 1) * pitch - r] + up[-r * pitch - r];
    const int diamond = ev[(t + 1) * pitch + 1] - od[-t] - od[t + 1] + ev[-t * pitch + 1];
    return square + diamond;
}

template <int... I>
__device__ __forceinline__ void star_sums(int (&vals)[N_SIZES], unsigned need, const int *up, const int *ev, const int *od, int pitch,
                                          std::integer_sequence<int, I...>)
{
    ((vals[I] = (need >> I) & 1u ? star_sum<I>(up, ev, od, pitch) : 0), ...);   // `need` is uniform
}

template <int P> __device__ __forceinline__ void star_pattern(const int (&vals)[N_SIZES], const Patterns &pt, float &best, int &size)
{
    if (P >= pt.npatterns)
        return;
    constexpr int o = PAIRS[P][0], i = PAIRS[P][1], o_size = SIZES0[o];
    const int inner = vals[i], outer = vals[o] - inner;
    const float a = (float)inner * pt.inv_inner[P], b = (float)outer * pt.inv_outer[P];
    const float r = a - b;
    if (fabsf(r) > fabsf(best)) {
        best = r;
        size = o_size;
    }
}

template <int... P>
__device__ __forceinline__ void star_patterns(const int (&vals)[N_SIZES], const Patterns &pt, float &best, int &size,
                                              std::integer_sequence<int, P...>)
{
    (star_pattern<P>(vals, pt, best, size), ...);
}

// a lane per pixel, a workgroup per 256 pixels of a row.  The largest offset from a pixel's entry is (t + 1) (pitch + 1) < 2^22.
__global__ __launch_bounds__(256) void star_response_kernel(const int *__restrict__ up_all, const int *__restrict__ even_all,
                                                            const int *__restrict__ odd_all, size_t stride, int w, int h, Patterns pt,
                                                            float *__restrict__ resp_all, int16_t *__restrict__ size_all)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= w)
        return;
    const size_t px = (size_t)w * h, at = (size_t)y * w + x;
    float best = 0.f;
    int size = 0;
    const int b = pt.border;
    if (x >= b && x < w - b && y >= b && y < h - b) {
        const int pitch = w + 1;
        const size_t e = blockIdx.z * stride + (size_t)y * pitch + x;
        int vals[N_SIZES];
        star_sums(vals, pt.need, up_all + e, even_all + e, odd_all + e, pitch, std::make_integer_sequence<int, N_SIZES>());
        star_patterns(vals, pt, best, size, std::make_integer_sequence<int, N_PAIRS>());
    }
    resp_all[blockIdx.z * px + at] = best;
    size_all[blockIdx.z * px + at] = (int16_t)size;
}

// ---------------------------------------------------------------------------------------------------------------- tiles
struct TileArgs {
    int w, h, border, delta, tiles_x;
    unsigned tiles;
    float threshold, line_projected;
    int line_binarized;
};

// the line test at (x, y): every sample is inside the image (star_plan_check.cpp: line_reach(sz) <= border)
__device__ bool star_on_line(const float *__restrict__ rp, const int16_t *__restrict__ sp, int w, int x, int y, int sz, float lt_proj, int lt_bin)
{
    const int d = sz / 4;
    float lxx = 0.f, lyy = 0.f, lxy = 0.f;
    for (int v = -4; v <= 4; v++)
        for (int u = -4; u <= 4; u++) {
            const float *q = rp + (size_t)(y + v * d) * w + (x + u * d);
            const float lx = q[1] - q[-1], ly = q[w] - q[-w];
            lxx += lx * lx;
            lyy += ly * ly;
            lxy += lx * ly;
        }
    const float s = lxx + lyy;
    if (s * s >= lt_proj * (lxx * lyy - lxy * lxy))
        return true;
    long long bxx = 0, byy = 0, bxy = 0;
    for (int v = -4; v <= 4; v++)
        for (int u = -4; u <= 4; u++) {
            const int16_t *q = sp + (size_t)(y + v * d) * w + (x + u * d);
            const int lx = (q[1] == sz) - (q[-1] == sz), ly = (q[w] == sz) - (q[-w] == sz);
            bxx += lx * lx;
            byy += ly * ly;
            bxy += lx * ly;
        }
    return (bxx + byy) * (bxx + byy) >= (long long)lt_bin * (bxx * byy - bxy * bxy);
}

// does the candidate at (x, y) with the extremum `ext` stay a key point?
template <bool MAXIMUM>
__device__ bool star_keep(const float *__restrict__ rp, const int16_t *__restrict__ sp, const TileArgs &a, int x, int y, float ext)
{
    const int ya = max(y - a.delta, 0), yb = min(y + a.delta, a.h - 1), xa = max(x - a.delta, 0), xb = min(x + a.delta, a.w - 1);
    for (int yy = ya; yy <= yb; yy++)
        for (int xx = xa; xx <= xb; xx++) {
            const float v = rp[(size_t)yy * a.w + xx];
            if ((MAXIMUM ? v >= ext : v <= ext) && (xx != x || yy != y))
                return false;
        }
    const int sz = sp[(size_t)y * a.w + x];
    if (sz < MIN_KEYPOINT_SIZE)
        return false;
    return !star_on_line(rp, sp, a.w, x, y, sz, a.line_projected, a.line_binarized);
}

// the word of a tile: bit 16 = its maximum is a key point, at pixel (bits 0-7) of the tile in row-major order; bit 17 and bits 8-15
// the same for its minimum.  A wavefront owns 64 consecutive tiles and leaves their key-point count.
__global__ __launch_bounds__(256) void star_tile_kernel(const float *__restrict__ resp_all, const int16_t *__restrict__ size_all, TileArgs a,
                                                        unsigned *__restrict__ tile_all, int *__restrict__ span_count_all, unsigned spans)
{
    const unsigned ti = blockIdx.x * 256u + threadIdx.x;
    const size_t px = (size_t)a.w * a.h;
    const float *__restrict__ rp = resp_all + blockIdx.y * px;
    const int16_t *__restrict__ sp = size_all + blockIdx.y * px;
    unsigned word = 0;
    if (ti < a.tiles) {
        const int step = a.delta + 1;
        const int ty = ti / (unsigned)a.tiles_x, tx = ti - (unsigned)ty * a.tiles_x;
        const int x0 = a.border + tx * step, y0 = a.border + ty * step;
        const int x1 = min(x0 + step, a.w - a.border), y1 = min(y0 + step, a.h - a.border);
        float hi = a.threshold, lo = -a.threshold;
        int pmax = -1, pmin = -1;
        for (int y = y0; y < y1; y++)
            for (int x = x0; x < x1; x++) {
                const float v = rp[(size_t)y * a.w + x];
                if (v > hi) {
                    hi = v;
                    pmax = (y - y0) * step + (x - x0);
                } else if (v < lo) {
                    lo = v;
                    pmin = (y - y0) * step + (x - x0);
                }
            }
        if (pmax >= 0 && star_keep<true>(rp, sp, a, x0 + pmax % step, y0 + pmax / step, hi))
            word |= 0x10000u | (unsigned)pmax;
        if (pmin >= 0 && star_keep<false>(rp, sp, a, x0 + pmin % step, y0 + pmin / step, lo))
            word |= 0x20000u | ((unsigned)pmin << 8);
        tile_all[blockIdx.y * (size_t)a.tiles + ti] = word;
    }
    const int count = __popcll(__ballot((word & 0x10000u) != 0)) + __popcll(__ballot((word & 0x20000u) != 0));
    const unsigned span = ti >> 6;
    if ((threadIdx.x & 63) == 0 && span < spans)
        span_count_all[blockIdx.y * (size_t)spans + span] = count;
}

// one workgroup per image: span_offset = exclusive scan of span_count, counts[img] = the total
__global__ __launch_bounds__(256) void star_scan_kernel(const int *__restrict__ span_count, int *__restrict__ span_offset, unsigned spans,
                                                        int *__restrict__ counts)
{
    __shared__ int s_wave[4];
    const int img = blockIdx.x;
    // spans <= 2^22: w, h <= 16384 and 64 tiles of at least a pixel per span
    const int total = svo::block_scan_counts<256>(span_count + (size_t)img * spans, span_offset + (size_t)img * spans, (int)spans, s_wave);
    if (threadIdx.x == 0)
        counts[img] = total;
}

// the tiles again: a key point goes to the wavefront's offset + the key points of the lanes below; a tile's maximum before its minimum
__global__ __launch_bounds__(256) void star_scatter_kernel(const unsigned *__restrict__ tile_all, const float *__restrict__ resp_all,
                                                           const int16_t *__restrict__ size_all, TileArgs a,
                                                           const int *__restrict__ span_offset_all, unsigned spans, int cap, size_t list_stride,
                                                           float *xy, float *ksize, float *kresp)
{
    const unsigned ti = blockIdx.x * 256u + threadIdx.x;
    const size_t px = (size_t)a.w * a.h;
    const unsigned word = ti < a.tiles ? tile_all[blockIdx.y * (size_t)a.tiles + ti] : 0u;
    const unsigned long long m1 = __ballot((word & 0x10000u) != 0), m2 = __ballot((word & 0x20000u) != 0);
    if (!(word & 0x30000u))
        return;
    int pos = span_offset_all[blockIdx.y * (size_t)spans + (ti >> 6)] + svo::lanes_below(m1) + svo::lanes_below(m2);
    const int step = a.delta + 1;
    const int ty = ti / (unsigned)a.tiles_x, tx = ti - (unsigned)ty * a.tiles_x;
    const int x0 = a.border + tx * step, y0 = a.border + ty * step;
    float *__restrict__ oxy = xy + 2 * blockIdx.y * list_stride;   // the caller's array: 4-byte alignment is all it has
    for (int k = 0; k < 2; k++) {
        if (!(word & (0x10000u << k)))
            continue;
        const int p = (word >> (8 * k)) & 0xffu;
        const int x = x0 + p % step, y = y0 + p / step;
        if (pos < cap) {
            oxy[2 * (size_t)pos] = (float)x;
            oxy[2 * (size_t)pos + 1] = (float)y;
            const size_t at = blockIdx.y * px + (size_t)y * a.w + x;
            if (ksize)
                ksize[blockIdx.y * list_stride + pos] = (float)size_all[at];
            if (kresp)
                kresp[blockIdx.y * list_stride + pos] = resp_all[at];
        }
        pos++;
    }
}

// ---------------------------------------------------------------------------------------------------------------- host side
int star_refuse(const char *fn, const char *why)
{
    svo_set_error("%s: %s", fn, why);
    return SVO_ERR_ARG;
}

int star_overflow(const char *fn, int w, int h)
{
    svo_set_error("%s: the int32 tables of %d x %d pixels could overflow (255 w h > 2^31 - 1)", fn, w, h);
    return SVO_ERR_CAPACITY;
}

// the tables and the two planes of nb device images into ctx->feat_sum, laid out by p
int star_planes(svo_ctx *ctx, const uint8_t *const *d_images, int nb, int w, int h, int c, const Plan &p)
{
    hipStream_t st = ctx->stream;
    if (p.table_stride != (size_t)integral_img_stride(w, h)) {
        svo_set_error("svo_star: the plan's table stride is not integral_scan.hip.h's");
        return SVO_ERR_STATE;
    }
    int rc;
    if ((rc = integral_images(ctx, d_images, nb, w, h, c, p.total - p.off_even)))
        return rc;
    uint8_t *wb = ctx->feat_sum.as<uint8_t>();
    int *up = reinterpret_cast<int *>(wb + p.off_upright), *ev = reinterpret_cast<int *>(wb + p.off_even);
    int *od = reinterpret_cast<int *>(wb + p.off_odd);
    const ImageBatch im = make_image_batch(d_images, nb);
    hipLaunchKernelGGL(star_diag_left_kernel, dim3((w + h + 1 + 255) / 256, nb), dim3(256), 0, st, im, w, h, c, ev, od, p.table_stride);
    hipLaunchKernelGGL(star_diag_right_kernel, dim3((w + h + 255) / 256, nb), dim3(256), 0, st, im, w, h, c, ev, od, p.table_stride);
    hipLaunchKernelGGL(star_col_scan_kernel, dim3((w + 1 + 63) / 64, nb, 2), dim3(64), 0, st, w, h, ev, od, p.table_stride);
    hipLaunchKernelGGL(star_response_kernel, dim3((w + 255) / 256, h, nb), dim3(256), 0, st, up, ev, od, p.table_stride, w, h,
                       make_patterns(p.lay), reinterpret_cast<float *>(wb + p.off_resp), reinterpret_cast<int16_t *>(wb + p.off_size));
    SVO_HIP(hipGetLastError());
    return SVO_OK;
}

}  // namespace

extern "C" {

void svo_star_default_params(svo_star_params *p)
{
    if (!p)
        return;
    p->max_size = 45;
    p->response_threshold = 30;
    p->line_threshold_projected = 10;
    p->line_threshold_binarized = 8;
    p->suppress_nonmax_size = 5;
}

int svo_star_layout(int w, int h, int max_size, int *npatterns, int *max_idx, int *border)
{
    SVO_CHECK_ARG(w >= 1 && h >= 1 && w <= MAX_DIM && h <= MAX_DIM);
    SVO_CHECK_ARG(max_size >= 3 && max_size <= 128);
    const Layout l = layout(w, h, max_size);
    if (npatterns)
        *npatterns = l.npatterns;
    if (max_idx)
        *max_idx = l.max_idx;
    if (border)
        *border = l.border;
    return SVO_OK;
}

int svo_star_detect_batch(svo_ctx *ctx, const uint8_t *const *images, int n_images, int w, int h, int c, const svo_star_params *prm,
                          int cap, float *xy, float *size, float *response, int *n, int mem)
{
    const char *fn = "svo_star_detect_batch";
    if (!ctx)
        return star_refuse(fn, "ctx must not be null");
    if (const char *why = check_args(images, prm, xy, n, n_images, w, h, c, cap))
        return star_refuse(fn, why);
    if (mem != SVO_MEM_HOST && mem != SVO_MEM_DEVICE)
        return star_refuse(fn, "mem must be SVO_MEM_HOST or SVO_MEM_DEVICE");
    if (!aligned4(xy) || !aligned4(size) || !aligned4(response) || !aligned4(n))
        return star_refuse(fn, "xy, size, response and n must be 4-byte aligned");
    for (int k = 0; k < n_images; k++)
        if (!images[k])
            return star_refuse(fn, "an image pointer is null");
    if (!fits_int32(w, h))
        return star_overflow(fn, w, h);
    const bool host = mem == SVO_MEM_HOST;
    const size_t px = (size_t)w * h;
    const size_t lcap = (size_t)cap < 2 * px ? (size_t)cap : 2 * px;   // a pixel is at most a maximum and a minimum
    const Plan p = make_plan(w, h, n_images, (int)lcap, prm, host);
    if (p.empty) {
        for (int k = 0; k < n_images; k++)
            n[k] = 0;
        return SVO_OK;
    }
    SVO_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint8_t *ptrs[MAX_BATCH];
    int rc;
    if ((rc = stage_images(ctx, images, n_images, px * c, mem, ptrs)) || (rc = star_planes(ctx, ptrs, n_images, w, h, c, p)))
        return rc;
    uint8_t *wb = ctx->feat_sum.as<uint8_t>();
    const float *d_resp = reinterpret_cast<const float *>(wb + p.off_resp);
    const int16_t *d_size = reinterpret_cast<const int16_t *>(wb + p.off_size);
    unsigned *d_tile = reinterpret_cast<unsigned *>(wb + p.off_tile);
    int *d_span_count = reinterpret_cast<int *>(wb + p.off_span_count), *d_span_offset = reinterpret_cast<int *>(wb + p.off_span_offset);
    int *d_counts = reinterpret_cast<int *>(wb + p.off_counts);
    float *d_xy = host ? reinterpret_cast<float *>(wb + p.off_xy) : xy;
    float *d_ksize = !size ? nullptr : host ? reinterpret_cast<float *>(wb + p.off_ksize) : size;
    float *d_kresp = !response ? nullptr : host ? reinterpret_cast<float *>(wb + p.off_kresp) : response;
    const size_t stride = host ? lcap : (size_t)cap;

    TileArgs a;
    a.w = w, a.h = h, a.border = p.lay.border, a.delta = p.delta, a.tiles_x = p.tiles_x, a.tiles = (unsigned)p.tiles;
    a.threshold = (float)prm->response_threshold, a.line_projected = (float)prm->line_threshold_projected;
    a.line_binarized = prm->line_threshold_binarized;
    const dim3 tgrid((unsigned)((p.tiles + 255) / 256), n_images);
    hipLaunchKernelGGL(star_tile_kernel, tgrid, dim3(256), 0, st, d_resp, d_size, a, d_tile, d_span_count, (unsigned)p.spans);
    hipLaunchKernelGGL(star_scan_kernel, dim3(n_images), dim3(256), 0, st, d_span_count, d_span_offset, (unsigned)p.spans, d_counts);
    hipLaunchKernelGGL(star_scatter_kernel, tgrid, dim3(256), 0, st, d_tile, d_resp, d_size, a, d_span_offset, (unsigned)p.spans, (int)lcap,
                       stride, d_xy, d_ksize, d_kresp);
    SVO_HIP(hipGetLastError());
    // the one wait of a detection: the counts
    if ((rc = read_counts(ctx, d_counts, n_images, n)))
        return rc;
    bool over = false;
    for (int k = 0; k < n_images; k++)
        over = over || n[k] > cap;
    if (host) {
        const HostColumn cols[3] = {{xy, d_xy, 8}, {size, d_ksize, 4}, {response, d_kresp, 4}};
        for (int k = 0; k < n_images; k++) {   // the staged lists are lcap rows apart, the caller's cap rows
            const size_t m = (size_t)(n[k] < cap ? n[k] : cap);
            for (int col = 0; m && col < 3; col++)
                if (cols[col].host)
                    SVO_HIP(hipMemcpyAsync(static_cast<uint8_t *>(cols[col].host) + (size_t)k * cap * cols[col].bytes,
                                           static_cast<const uint8_t *>(cols[col].dev) + k * stride * cols[col].bytes, m * cols[col].bytes,
                                           hipMemcpyDeviceToHost, st));
        }
        SVO_HIP(hipStreamSynchronize(st));
    }
    if (over) {
        svo_set_error("%s: an image has more than cap = %d key points (n[] holds the counts)", fn, cap);
        return SVO_ERR_CAPACITY;
    }
    return SVO_OK;
}

int svo_star_responses(svo_ctx *ctx, const uint8_t *image, int w, int h, int c, const svo_star_params *prm, float *response,
                       int16_t *size, int *border, int mem)
{
    const char *fn = "svo_star_responses";
    if (!ctx || !image || !response || !size || !border)
        return star_refuse(fn, "ctx, image, response, size and border must not be null");
    if (const char *why = check_params(prm))
        return star_refuse(fn, why);
    if (const char *why = check_image(w, h, c))
        return star_refuse(fn, why);
    if (mem != SVO_MEM_HOST && mem != SVO_MEM_DEVICE)
        return star_refuse(fn, "mem must be SVO_MEM_HOST or SVO_MEM_DEVICE");
    if (!aligned4(response) || (reinterpret_cast<uintptr_t>(size) & 1u) || !aligned4(border))
        return star_refuse(fn, "response and border must be 4-byte aligned, size 2-byte aligned");
    if (!fits_int32(w, h))
        return star_overflow(fn, w, h);
    const bool host = mem == SVO_MEM_HOST;
    const size_t px = (size_t)w * h;
    const Plan p = make_plan(w, h, 1, 1, prm, false);
    SVO_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (p.empty) {
        if (host) {
            memset(response, 0, px * 4);
            memset(size, 0, px * 2);
        } else {
            SVO_HIP(hipMemsetAsync(response, 0, px * 4, st));
            SVO_HIP(hipMemsetAsync(size, 0, px * 2, st));
        }
        *border = p.lay.border;
        return SVO_OK;
    }
    const uint8_t *d_img = nullptr;
    int rc;
    if ((rc = stage_images(ctx, &image, 1, px * c, mem, &d_img)) || (rc = star_planes(ctx, &d_img, 1, w, h, c, p)))
        return rc;
    const uint8_t *wb = ctx->feat_sum.as<uint8_t>();
    const hipMemcpyKind kind = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    SVO_HIP(hipMemcpyAsync(response, wb + p.off_resp, px * 4, kind, st));
    SVO_HIP(hipMemcpyAsync(size, wb + p.off_size, px * 2, kind, st));
    if (host)
        SVO_HIP(hipStreamSynchronize(st));
    *border = p.lay.border;   // last: a call that fails leaves it alone
    return SVO_OK;
}

}  // extern "C"
