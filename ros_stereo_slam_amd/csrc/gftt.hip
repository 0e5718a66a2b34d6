// gftt.hip -- cv::goodFeaturesToTrack (Shi-Tomasi min-eigenvalue or Harris corners) as a key-point source, for gfx950.
//
// The definition is the one tests/gftt_numpy.py states, points G1 ... G13: Sobel derivatives of the grey
// image in float, their products summed over a blockSize window in double in row-major order, the corner measure, the cut at
// qualityLevel times the image's (masked) maximum, 3 x 3 local maxima one pixel inside the border, the total order (value
// descending, row-major index descending) and the greedy minimum-distance selection.  Every float operation is written as the
// restatement writes it and nothing is fused.
//
// Launches of one call, the image index on a grid axis or in the sort key (up to 16 images of one size):
//   gftt_eig_kernel        a 64 x 16 tile: the grey pixels with a halo of 1 + blockSize / 2 in LDS (BGR converted while staging, the
//                          border mirrored), dx and dy of the tile and its box halo in LDS (a product outside the image is the
//                          product at the mirrored pixel), the box sums and the measure; writes the measure plane and raises the
//                          image's maximum: an order-preserving integer key under atomicMax, the same whatever the order of the
//                          workgroups
//   gftt_cand_kernel       <false>: a wavefront counts the candidates among its 1024 consecutive pixels (threshold, 3 x 3 maximum of
//                          the thresholded plane, the candidate test); gftt_cand_scan_kernel: one workgroup scans all the counts of
//                          the batch, image-major; <true>: every candidate's 64-bit key (image | ~value | ~index) written at its
//                          row-major rank -- no atomic decides a position
//   radix_sort_pairs       cloud_index.hip.h: the keys are unique, so ascending order is the recipe's total order, image by image
//   gftt_bin_kernel, gftt_cell_scan_kernel, gftt_fill_kernel   (min_distance >= 1) the ranked candidates of an image listed by cell
//                          of cvRound(min_distance) pixels; the order inside a cell's list is whatever the atomics give, and nothing
//                          depends on it
//   gftt_select_kernel     one workgroup per image.  Rounds separated by workgroup barriers: an undecided candidate is rejected if
//                          an accepted one lies within the distance, accepted if no undecided candidate of earlier rank does, and
//                          waits otherwise.  The best-ranked undecided candidate decides in every round, so the rounds end after at
//                          most n, with exactly the sequential greedy result; no workgroup waits for another.  Then the accepted
//                          ones are compacted in rank order, the first max_corners of them written.
// The host waits twice: for the candidate counts (the sort is launched for their sum) and for the corner counts.
#include "cloud_index.hip.h"
#include "gftt_plan.hip.h"

#pragma clang fp contract(off)

namespace {

#include "feature_batch.hip.h"

using namespace gftt_plan;
static_assert(MAX_BATCH == IMAGE_MAXBATCH, "one image table for every batched entry point");
static_assert(SORT_TILE == RS_TILE, "the histogram array of the plan is sized for the sort's tile");
static_assert(TILE_W == 64 && TILE_H % 4 == 0, "a wavefront spans a tile row; the workgroup's four wavefronts step four rows");

struct MaskBatch {
    const uint8_t *m[MAX_BATCH];   // null: no mask for the image
};

// cv::borderInterpolate(p, n, BORDER_REFLECT_101)
__device__ __forceinline__ int reflect101(int p, int n)
{
    if (n == 1)
        return 0;
    while (p < 0 || p >= n)
        p = p < 0 ? -p : 2 * n - 2 - p;
    return p;
}

__device__ __forceinline__ unsigned wave_max_key(unsigned v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        v = max(v, (unsigned)__shfl_xor((int)v, o, 64));
    return v;
}

// ---------------------------------------------------------------------------------------------------------------- measure
// G5 on the three box sums
__device__ __forceinline__ float corner_measure(float cxx, float cxy, float cyy, int harris, float kf)
{
    if (harris) {
        const float det = (cxx * cyy) - (cxy * cxy), tr = cxx + cyy;
        return det - (kf * tr) * tr;
    }
    const float a = cxx * 0.5f, b = cxy, c = cyy * 0.5f;
    const float d = a - c;
    return (a + c) - sqrtf(d * d + b * b);
}

// dynamic LDS: dx[DH][DW], dy[DH][DW] floats, then grey[GH][GW] bytes; B = block / 2, R = B + 1, DW = 64 + 2 B, GW = 64 + 2 R
__global__ __launch_bounds__(256) void gftt_eig_kernel(ImageBatch src, MaskBatch masks, int w, int h, int c, int block, float k1, float k0,
                                                       int harris, float kf, float *eig, unsigned *max_key)
{
    extern __shared__ float lds[];
    const int B = block >> 1, R = B + 1;
    const int DW = TILE_W + 2 * B, DH = TILE_H + 2 * B, GW = TILE_W + 2 * R, GH = TILE_H + 2 * R;
    float *sdx = lds, *sdy = lds + DW * DH;
    uint8_t *grey = reinterpret_cast<uint8_t *>(lds + 2 * DW * DH);
    const int x0 = blockIdx.x * TILE_W, y0 = blockIdx.y * TILE_H, img = blockIdx.z;
    const uint8_t *__restrict__ s = src.img[img];
    // G1: the grey pixels of the tile and its halo, the image's border mirrored
    for (int i = threadIdx.x; i < GW * GH; i += 256) {
        const int ly = i / GW, lx = i - ly * GW;
        const int gy = reflect101(y0 - R + ly, h), gx = reflect101(x0 - R + lx, w);
        const size_t p = (size_t)gy * w + gx;
        grey[i] = (uint8_t)(c == 1 ? s[p] : svo_bgr2gray(s[3 * p], s[3 * p + 1], s[3 * p + 2]));
    }
    __syncthreads();
    // G2: dx and dy at the pixels of the tile and of its box halo; outside the image the derivative of the mirrored PIXEL
    for (int i = threadIdx.x; i < DW * DH; i += 256) {
        const int ly = i / DW, lx = i - ly * DW;
        const int qy = reflect101(y0 - B + ly, h) - (y0 - R), qx = reflect101(x0 - B + lx, w) - (x0 - R);
        float dx = 0.f, dy = 0.f;
        // always true for the pixels a box sum of this tile reads; the rest of a partial tile's halo is not read
        if (qx >= 1 && qx <= GW - 2 && qy >= 1 && qy <= GH - 2) {
            const uint8_t *g = grey + qy * GW + qx;
            const float a0 = g[-GW - 1], a1 = g[-GW], a2 = g[-GW + 1], b0 = g[-1], b2 = g[1], c0 = g[GW - 1], c1 = g[GW], c2 = g[GW + 1];
            const float ra = a2 - a0, rb = b2 - b0, rc = c2 - c0;
            dx = (ra + rc) * k1 + rb * k0;
            const float sa = (a0 + a2) * k1 + a1 * k0, sc = (c0 + c2) * k1 + c1 * k0;
            dy = sc - sa;
        }
        sdx[i] = dx;
        sdy[i] = dy;
    }
    __syncthreads();
    // G3 ... G5: the products summed over the window in double, row-major, rounded to float once
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int x = x0 + tx;
    const uint8_t *__restrict__ mk = masks.m[img];
    float *__restrict__ out = eig + (size_t)img * w * h;
    unsigned best = 0;
#pragma unroll 1
    for (int k = 0; k < TILE_H / 4; k++) {
        const int ly = ty + 4 * k, y = y0 + ly;
        if (x >= w || y >= h)
            continue;
        double sxx = 0., sxy = 0., syy = 0.;
        for (int j = 0; j < block; j++) {
            const float *px = sdx + (ly + j) * DW + tx, *py = sdy + (ly + j) * DW + tx;
            for (int i = 0; i < block; i++) {
                const float a = px[i], b = py[i];
                const float aa = a * a, ab = a * b, bb = b * b;
                sxx += (double)aa;
                sxy += (double)ab;
                syy += (double)bb;
            }
        }
        const float v = corner_measure((float)sxx, (float)sxy, (float)syy, harris, kf);
        const size_t p = (size_t)y * w + x;
        out[p] = v;
        if (max_key && (!mk || mk[p]))
            best = max(best, float_key(v));
    }
    if (max_key) {   // kernel-uniform
        best = wave_max_key(best);
        if (tx == 0 && best)
            atomicMax(&max_key[img], best);
    }
}

// ---------------------------------------------------------------------------------------------------------------- candidates
// 0, or the thresholded measure of a candidate (G7 ... G9); never 0 for a candidate
__device__ __forceinline__ float gftt_candidate(const float *__restrict__ e, const uint8_t *__restrict__ mk, int w, int h, int x, int y,
                                                float t)
{
    if (x < 1 || y < 1 || x > w - 2 || y > h - 2)
        return 0.f;
    const float *q = e + (size_t)y * w + x;
    const float v = q[0] > t ? q[0] : 0.f;
    if (v == 0.f || (mk && !mk[(size_t)y * w + x]))
        return 0.f;
    float m = v;
#pragma unroll
    for (int j = -1; j <= 1; j++)
#pragma unroll
        for (int i = -1; i <= 1; i++) {
            const float u = q[j * w + i];
            m = fmaxf(m, u > t ? u : 0.f);
        }
    return v == m ? v : 0.f;
}

template <bool SCATTER>
__global__ __launch_bounds__(64 * WAVES) void gftt_cand_kernel(const float *eig, MaskBatch masks, int w, int h, const unsigned *max_key,
                                                              double quality, int spans, int *span_count, const int *span_offset,
                                                              uint64_t *keys, int *vals)
{
    const int img = blockIdx.y, lane = threadIdx.x & 63;
    const int span = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (span >= spans)   // wave-uniform
        return;
    const float *__restrict__ e = eig + (size_t)img * w * h;
    const uint8_t *__restrict__ mk = masks.m[img];
    const unsigned mkey = max_key[img];
    const float t = quality_cut(mkey ? key_float(mkey) : 0.f, quality);   // G6: nothing seen = 0
    const unsigned npix = (unsigned)w * (unsigned)h;   // <= 2^28
    int base = SCATTER ? span_offset[(size_t)img * spans + span] : 0;
    for (int i = 0; i < SPAN / 64; i++) {
        const unsigned idx = (unsigned)span * SPAN + i * 64 + lane;
        float v = 0.f;
        if (idx < npix) {
            const int y = idx / (unsigned)w, x = idx - (unsigned)y * w;
            v = gftt_candidate(e, mk, w, h, x, y, t);
        }
        const unsigned long long m = __ballot(v != 0.f);
        if (SCATTER && v != 0.f) {
            const int pos = base + svo::lanes_below(m);   // < the interior pixels of the batch: inside the arrays
            keys[pos] = sort_key(img, v, idx);
            vals[pos] = (int)idx;
        }
        base += __popcll(m);
    }
    if (!SCATTER && lane == 0)
        span_count[(size_t)img * spans + span] = base;
}

// one workgroup: the exclusive scan of all the span counts of the batch, image-major, in place; base[i] = where image i's candidates
// start, base[n_images] = their number
__global__ __launch_bounds__(256) void gftt_cand_scan_kernel(int *span, int spans, int n_images, int *base)
{
    __shared__ int s_wave[4];
    const int total = svo::block_scan_counts<256>(span, span, spans * n_images, s_wave);
    __syncthreads();
    if ((int)threadIdx.x < n_images)
        base[threadIdx.x] = span[(size_t)threadIdx.x * spans];
    if (threadIdx.x == 0)
        base[n_images] = total;
}

// ---------------------------------------------------------------------------------------------------------------- selection
__device__ __forceinline__ int pack_xy(int x, int y) { return x | (y << 16); }

// one lane per sorted candidate: its pixel, its state, and one more in its cell's count
__global__ __launch_bounds__(256) void gftt_bin_kernel(const uint64_t *keys, const int *base, int n_images, int w, int cell, int grid_w,
                                                       int cells, int *pxy, int *state, int *cell_count)
{
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= base[n_images])
        return;
    const uint64_t k = keys[g];
    const unsigned idx = key_index(k);
    const int y = idx / (unsigned)w, x = idx - (unsigned)y * w;
    pxy[g] = pack_xy(x, y);
    state[g] = 0;
    if (cell_count)
        atomicAdd(&cell_count[(size_t)key_image(k) * (cells + 1) + (y / cell) * grid_w + x / cell], 1);   // counts only
}

__global__ __launch_bounds__(256) void gftt_cell_scan_kernel(int *cell_start, int cells)
{
    __shared__ int s_wave[4];
    int *c = cell_start + (size_t)blockIdx.x * (cells + 1);
    const int total = svo::block_scan_counts<256>(c, c, cells, s_wave);
    if (threadIdx.x == 0)
        c[cells] = total;
}

// members of image i, [base[i] + cell_start[cell], ...): the ranks (inside the image) of the candidates of the cell
__global__ __launch_bounds__(256) void gftt_fill_kernel(const uint64_t *keys, const int *pxy, const int *base, int n_images, int cell,
                                                        int grid_w, int cells, const int *cell_start, int *cell_cursor, int *members)
{
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= base[n_images])
        return;
    const int img = key_image(keys[g]), p = pxy[g];
    const int cid = ((p >> 16) / cell) * grid_w + (p & 0xffff) / cell;
    const int at = cell_start[(size_t)img * (cells + 1) + cid] + atomicAdd(&cell_cursor[(size_t)img * cells + cid], 1);
    members[base[img] + at] = g - base[img];   // at < the image's candidates
}

// state of a candidate: 0 undecided, else (round << 2) | 1 accepted / 2 rejected.  A reader in round r takes a state written in round
// r for undecided: every decision of a round is made on the states the round began with.
__global__ __launch_bounds__(SELECT_T) void gftt_select_kernel(const uint64_t *keys, const int *pxy_all, int *state_all, const int *base,
                                                              int select, int cell, int grid_w, int grid_h, const int *cell_start_all,
                                                              const int *members_all, double md2, int max_corners, int cap,
                                                              size_t stride, float *xy, float *resp, int *counts)
{
    __shared__ int s_wave[SELECT_T / 64];
    __shared__ int s_undecided;
    const int img = blockIdx.x, tid = threadIdx.x;
    const int b0 = base[img], n = base[img + 1] - b0;
    const int *__restrict__ pxy = pxy_all + b0;
    int *state = state_all + b0;
    if (select) {
        const int *__restrict__ cs = cell_start_all + (size_t)img * (grid_w * grid_h + 1);
        const int *__restrict__ members = members_all + b0;
        for (int round = 1;; round++) {   // at most n rounds: the best-ranked undecided candidate decides
            if (tid == 0)
                s_undecided = 0;
            __syncthreads();
            int waiting = 0;
            for (int r = tid; r < n; r += SELECT_T) {
                if (__hip_atomic_load(&state[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))
                    continue;
                const int p = pxy[r], x = p & 0xffff, y = p >> 16;
                const int cx = x / cell, cy = y / cell;
                int verdict = 1;
                for (int yy = max(cy - 1, 0); yy <= min(cy + 1, grid_h - 1) && verdict != 2; yy++)
                    for (int xx = max(cx - 1, 0); xx <= min(cx + 1, grid_w - 1) && verdict != 2; xx++) {
                        const int cid = yy * grid_w + xx;
                        for (int m = cs[cid]; m < cs[cid + 1]; m++) {
                            const int q = members[m];
                            if (q == r)
                                continue;
                            const int pq = pxy[q];
                            const float dx = (float)x - (float)(pq & 0xffff), dy = (float)y - (float)(pq >> 16);
                            const float d2 = dx * dx + dy * dy;
                            if (!((double)d2 < md2))
                                continue;
                            const int sq = __hip_atomic_load(&state[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                            if (sq && (sq >> 2) < round) {
                                if ((sq & 3) == 1) {   // an accepted corner within the distance: it ranks before r
                                    verdict = 2;
                                    break;
                                }
                            } else if (q < r) {
                                verdict = 0;
                            }
                        }
                    }
                if (verdict)
                    __hip_atomic_store(&state[r], (round << 2) | verdict, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                else
                    waiting++;
            }
            if (waiting)
                atomicAdd(&s_undecided, waiting);   // a count: no order depends on it
            __syncthreads();
            const int left = s_undecided;
            __syncthreads();
            if (!left)   // uniform over the workgroup
                break;
        }
    }
    // the accepted candidates in rank order, the first max_corners of them
    const int limit = max_corners > 0 ? max_corners : 0x7fffffff;
    float2 *__restrict__ oxy = reinterpret_cast<float2 *>(xy) + img * stride;
    float *__restrict__ orp = resp ? resp + img * stride : nullptr;
    int carry = 0;
    for (int b = 0; b < n; b += SELECT_T) {
        const int r = b + tid;
        const bool a = r < n && (!select || (__hip_atomic_load(&state[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) & 3) == 1);
        int total;
        const int pos = carry + svo::block_excl_scan<SELECT_T>(a ? 1 : 0, s_wave, &total);
        if (a && pos < limit && pos < cap) {
            const int p = pxy[r];
            oxy[pos] = make_float2((float)(p & 0xffff), (float)(p >> 16));
            if (orp)
                orp[pos] = key_value(keys[b0 + r]);
        }
        carry += total;
        __syncthreads();   // s_wave is free for the next chunk
    }
    if (tid == 0)
        counts[img] = min(carry, limit);
}

int gftt_refuse(const char *fn, const char *why)
{
    svo_set_error("%s: %s", fn, why);
    return SVO_ERR_ARG;
}

// the eig launch of a call; max_key: null for svo_gftt_response
void launch_eig(hipStream_t st, const Plan &p, const ImageBatch &im, const MaskBatch &mk, const svo_gftt_params *prm, float *d_eig,
                unsigned *d_max)
{
    const double scale = 1.0 / (4.0 * prm->block_size * 255.0);   // G2
    hipLaunchKernelGGL(gftt_eig_kernel, dim3(p.tiles_x, p.tiles_y, p.n_images), dim3(256), p.eig_lds, st, im, mk, p.w, p.h, p.c,
                       prm->block_size, (float)scale, (float)(2.0 * scale), prm->use_harris != 0, (float)prm->k, d_eig, d_max);
}

int gftt_detect(const char *fn, svo_ctx *ctx, const uint8_t *const *images, const uint8_t *const *masks, int n_images, int w, int h, int c,
                const svo_gftt_params *prm, int cap, float *xy, float *response, int *n, int mem)
{
    if (!ctx)
        return gftt_refuse(fn, "ctx must not be null");
    if (const char *why = check_args(images, prm, xy, n, n_images, w, h, c, cap))
        return gftt_refuse(fn, why);
    if (mem != SVO_MEM_HOST && mem != SVO_MEM_DEVICE)
        return gftt_refuse(fn, "mem must be SVO_MEM_HOST or SVO_MEM_DEVICE");
    if (!aligned4(xy) || !aligned4(response) || !aligned4(n))
        return gftt_refuse(fn, "xy, response and n must be 4-byte aligned");
    for (int k = 0; k < n_images; k++)
        if (!images[k])
            return gftt_refuse(fn, "an image pointer is null");
    if (w < 3 || h < 3) {   // no pixel is one inside the border
        for (int k = 0; k < n_images; k++)
            n[k] = 0;
        return SVO_OK;
    }
    const bool host = mem == SVO_MEM_HOST;
    SVO_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t px = (size_t)w * h, interior = (size_t)(w - 2) * (h - 2);
    bool any_mask = false;
    for (int k = 0; masks && k < n_images; k++)
        any_mask = any_mask || masks[k];
    const uint8_t *ptrs[MAX_BATCH];
    int rc;
    if ((rc = stage_images(ctx, images, n_images, px * c, mem, ptrs)))
        return rc;
    const int lcap = (size_t)cap < interior ? cap : (int)interior;   // no image has more corners than interior pixels
    const Plan p = make_plan(w, h, c, n_images, lcap, prm, true, host, any_mask);
    if ((rc = ctx->gftt_work.ensure(p.total)))
        return rc;
    uint8_t *wb = ctx->gftt_work.as<uint8_t>();
    auto ints = [wb](size_t off) { return reinterpret_cast<int *>(wb + off); };
    unsigned *d_max = reinterpret_cast<unsigned *>(wb + p.off_max);
    int *d_base = ints(p.off_base), *d_counts = ints(p.off_counts), *d_span = ints(p.off_span);
    float *d_eig = reinterpret_cast<float *>(wb + p.off_eig);
    uint64_t *k0 = reinterpret_cast<uint64_t *>(wb + p.off_k0), *k1 = reinterpret_cast<uint64_t *>(wb + p.off_k1);
    int *v0 = ints(p.off_v0), *v1 = ints(p.off_v1);
    float *d_xy = host ? reinterpret_cast<float *>(wb + p.off_xy) : xy;
    float *d_resp = host ? reinterpret_cast<float *>(wb + p.off_resp) : response;
    const size_t stride = host ? (size_t)lcap : (size_t)cap;

    const ImageBatch im = make_image_batch(ptrs, n_images);
    MaskBatch mk{};
    for (int k = 0; k < n_images; k++) {
        const uint8_t *m = masks ? masks[k] : nullptr;
        if (m && host) {
            uint8_t *d = wb + p.off_mask + (size_t)k * px;
            SVO_HIP(hipMemcpyAsync(d, m, px, hipMemcpyHostToDevice, st));
            m = d;
        }
        mk.m[k] = m;
    }
    SVO_HIP(hipMemsetAsync(d_max, 0, sizeof(unsigned) * MAX_BATCH, st));
    launch_eig(st, p, im, mk, prm, d_eig, d_max);
    const dim3 cgrid(p.groups, n_images), cblock(64 * WAVES);
    hipLaunchKernelGGL(gftt_cand_kernel<false>, cgrid, cblock, 0, st, d_eig, mk, w, h, d_max, prm->quality_level, p.spans, d_span,
                       (const int *)nullptr, (uint64_t *)nullptr, (int *)nullptr);
    hipLaunchKernelGGL(gftt_cand_scan_kernel, dim3(1), dim3(256), 0, st, d_span, p.spans, n_images, d_base);
    hipLaunchKernelGGL(gftt_cand_kernel<true>, cgrid, cblock, 0, st, d_eig, mk, w, h, d_max, prm->quality_level, p.spans, (int *)nullptr,
                       d_span, k0, v0);
    SVO_HIP(hipGetLastError());
    // the first wait: the sort is launched for the number of candidates there are
    int *pin = reinterpret_cast<int *>(ctx->pinned);
    SVO_HIP(hipMemcpyAsync(pin, d_base, sizeof(int) * (n_images + 1), hipMemcpyDeviceToHost, st));
    SVO_HIP(hipStreamSynchronize(st));
    const int total = pin[n_images];
    if (total < 0 || (size_t)total > p.max_cand) {
        svo_set_error("%s: %d candidates counted, the bound is %zu", fn, total, p.max_cand);
        return SVO_ERR_HIP;
    }
    if ((rc = radix_sort_pairs(st, k0, v0, k1, v1, total, reinterpret_cast<unsigned *>(wb + p.off_hist))))
        return rc;
    int *d_pxy = ints(p.off_pxy), *d_state = ints(p.off_state), *d_cell_start = ints(p.off_cell_start);
    int *d_cursor = ints(p.off_cell_cursor), *d_members = ints(p.off_members);
    if (total) {
        const dim3 grid((total + 255) / 256);
        if (p.select) {
            SVO_HIP(hipMemsetAsync(d_cell_start, 0, sizeof(int) * n_images * ((size_t)p.cells + 1), st));
            SVO_HIP(hipMemsetAsync(d_cursor, 0, sizeof(int) * n_images * (size_t)p.cells, st));
        }
        hipLaunchKernelGGL(gftt_bin_kernel, grid, dim3(256), 0, st, k0, d_base, n_images, w, p.select ? p.cell : 1, p.grid_w, p.cells,
                           d_pxy, d_state, p.select ? d_cell_start : (int *)nullptr);
        if (p.select) {
            hipLaunchKernelGGL(gftt_cell_scan_kernel, dim3(n_images), dim3(256), 0, st, d_cell_start, p.cells);
            hipLaunchKernelGGL(gftt_fill_kernel, grid, dim3(256), 0, st, k0, d_pxy, d_base, n_images, p.cell, p.grid_w, p.cells,
                               d_cell_start, d_cursor, d_members);
        }
    }
    hipLaunchKernelGGL(gftt_select_kernel, dim3(n_images), dim3(SELECT_T), 0, st, k0, d_pxy, d_state, d_base, p.select, p.select ? p.cell : 1,
                       p.grid_w, p.grid_h, d_cell_start, d_members, prm->min_distance * prm->min_distance, prm->max_corners,
                       (int)(stride < (size_t)cap ? stride : (size_t)cap), stride, d_xy, d_resp, d_counts);
    SVO_HIP(hipGetLastError());
    SVO_HIP(hipMemcpyAsync(pin, d_counts, sizeof(int) * n_images, hipMemcpyDeviceToHost, st));
    SVO_HIP(hipStreamSynchronize(st));
    bool over = false;
    for (int k = 0; k < n_images; k++) {
        n[k] = pin[k];
        over = over || n[k] > cap;
    }
    if (host)
        for (int k = 0; k < n_images; k++) {
            const size_t m = (size_t)(n[k] < cap ? n[k] : cap);
            if (!m)
                continue;
            SVO_HIP(hipMemcpyAsync(xy + (size_t)k * cap * 2, d_xy + k * stride * 2, m * 8, hipMemcpyDeviceToHost, st));
            if (response)
                SVO_HIP(hipMemcpyAsync(response + (size_t)k * cap, d_resp + k * stride, m * 4, hipMemcpyDeviceToHost, st));
        }
    if (host)
        SVO_HIP(hipStreamSynchronize(st));
    if (over) {
        svo_set_error("%s: an image has more than cap = %d corners (n[] holds the counts)", fn, cap);
        return SVO_ERR_CAPACITY;
    }
    return SVO_OK;
}

}  // namespace

extern "C" {

void svo_gftt_default_params(svo_gftt_params *p)
{
    if (!p)
        return;
    p->max_corners = 1000;
    p->block_size = 3;
    p->use_harris = 0;
    p->pad = 0;
    p->quality_level = 0.01;
    p->min_distance = 1.0;
    p->k = 0.04;
}

int svo_gftt_detect_batch(svo_ctx *ctx, const uint8_t *const *images, const uint8_t *const *masks, int n_images, int w, int h, int c,
                          const svo_gftt_params *prm, int cap, float *xy, float *response, int *n, int mem)
{
    return gftt_detect("svo_gftt_detect_batch", ctx, images, masks, n_images, w, h, c, prm, cap, xy, response, n, mem);
}

int svo_gftt_response(svo_ctx *ctx, const uint8_t *image, int w, int h, int c, const svo_gftt_params *prm, float *eig, int mem)
{
    const char *fn = "svo_gftt_response";
    if (!ctx || !image || !prm || !eig)
        return gftt_refuse(fn, "ctx, image, prm and eig must not be null");
    if (const char *why = check_size(w, h, c, 1))
        return gftt_refuse(fn, why);
    if (const char *why = check_params(prm))
        return gftt_refuse(fn, why);
    if (mem != SVO_MEM_HOST && mem != SVO_MEM_DEVICE)
        return gftt_refuse(fn, "mem must be SVO_MEM_HOST or SVO_MEM_DEVICE");
    if (!aligned4(eig))
        return gftt_refuse(fn, "eig must be 4-byte aligned");
    const bool host = mem == SVO_MEM_HOST;
    SVO_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint8_t *ptrs[MAX_BATCH];
    int rc;
    if ((rc = stage_images(ctx, &image, 1, (size_t)w * h * c, mem, ptrs)))
        return rc;
    const Plan p = make_plan(w, h, c, 1, 1, prm, false, host, false);
    if ((rc = ctx->gftt_work.ensure(p.total)))
        return rc;
    float *d_eig = host ? reinterpret_cast<float *>(ctx->gftt_work.as<uint8_t>() + p.off_eig) : eig;
    launch_eig(st, p, make_image_batch(ptrs, 1), MaskBatch{}, prm, d_eig, nullptr);
    SVO_HIP(hipGetLastError());
    if (host) {
        SVO_HIP(hipMemcpyAsync(eig, d_eig, sizeof(float) * (size_t)w * h, hipMemcpyDeviceToHost, st));
        SVO_HIP(hipStreamSynchronize(st));
    }
    return SVO_OK;
}

}  // extern "C"
