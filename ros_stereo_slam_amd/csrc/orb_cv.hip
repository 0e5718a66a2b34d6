// orb_cv.hip -- cv::ORB's own shape on gfx950, N images per launch.
//
// What ORB::create()->detectAndCompute runs in visualSLAM::checkLoopDetectorStatus (src/optimizationStuff.cpp:49-56) with
// ORB::create()'s defaults -- 500 features, 8 levels of scale 1.2, FAST-9/16 at threshold 20 with its own score-based
// non-maximum suppression, retainBest(2 x quota) by that score, Harris 7x7 ranking, retainBest(quota), intensity-centroid
// orientation through fastAtan2, 256 rotated tests on the 7x7 / sigma 2 Gaussian of the level -- so that a DBoW2 vocabulary
// trained on cv::ORB descriptors (orb_voc00.yml.gz, include/visualSLAM.h:131-134) is usable once the learned 256 x 4
// sampling pattern is set through svo_orb_set_pattern.  The recipe is stated in full in oracle/orb.c
// (orc_orb_extract_cv), which this file matches bit for bit: everything is integer arithmetic plus a few individually
// rounded float operations.
//
// Layout: the 8 levels of an image back to back, unpadded (key points keep a 31-pixel margin, so no stage reads outside a
// level except the blur, which reflects); every work buffer holds `batch` images side by side.  blockIdx.z (or .y) carries
// (image, level), so ONE set of 11 launches serves up to 32 images (a launch per image was 11 launches + 6
// copies for 117 us of kernels).  Per image of 1241 x 376: 1.44 M pixels over the levels.
//   gray            image -> level 0
//   resize (x7)     level l from level l - 1: cv::resize INTER_LINEAR, 11-bit fixed point (a dependent chain by nature)
//   blur_corners    a workgroup per 128 x 16 tile: Gaussian 7x7 (exact integer sums, one rounding), the FAST corner score of the
//                   tile and one pixel around it, the 3x3 suppression; the survivors appended to the level's candidate list
//   select          one workgroup per (image, level): score histogram -> retainBest(2q) cut, Harris of the survivors,
//                   q-th largest response a byte at a time, raster-order write
//   describe        one wavefront per key point: disc moments, fastAtan2, the 256 tests from __ballot
#include <cmath>
#include <cstring>
#include <type_traits>
#include <vector>

#include "svo_internal.h"
#include "fast_atan2.hip.h"
#include "wave_ops.hip.h"

namespace {

constexpr int CV_EDGE = 31, CV_MAXLEV = 8, CV_MAXBATCH = 32;

struct CvLevels {
    int n_lev, n_features;
    int w[CV_MAXLEV], h[CV_MAXLEV], want[CV_MAXLEV], on[CV_MAXLEV];
    int pix_off[CV_MAXLEV], cand_off[CV_MAXLEV], cand_cap[CV_MAXLEV];
    float scale[CV_MAXLEV];
    int pix_total, cand_total;   // per image
    int rs_x[CV_MAXLEV], rs_y[CV_MAXLEV];                   // level l's column / row entries in the resize table
};

struct CvImages {
    const uint8_t *img[CV_MAXBATCH];
};

__global__ __launch_bounds__(256) void cv_gray_kernel(CvImages im, int n, int c, uint8_t *__restrict__ levels, int pix_total)
{
    // four pixels per thread: three dwords in (BGR; the image base is a device allocation or an image-sized multiple of
    // it), one dword out
    const int i = 4 * (blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n)
        return;
    const uint8_t *__restrict__ img = im.img[blockIdx.y];
    uint8_t *__restrict__ dst = levels + (size_t)blockIdx.y * pix_total + i;
    if (i + 3 < n) {
        unsigned out;
        if (c == 1) {
            __builtin_memcpy(&out, img + i, 4);
        } else {
            unsigned d[3];
            __builtin_memcpy(d, img + 3 * (size_t)i, 12);
            auto byte = [&](int k) { return (d[k >> 2] >> (8 * (k & 3))) & 0xffu; };
            out = 0;
#pragma unroll
            for (int j = 0; j < 4; j++)
                out |= ((1868u * byte(3 * j) + 9617u * byte(3 * j + 1) + 4899u * byte(3 * j + 2) + 8192u) >> 14) << (8 * j);
        }
        *reinterpret_cast<unsigned *>(dst) = out;   // level 0 of an image starts at a multiple of 64
    } else {
        for (int j = 0; i + j < n; j++)
            dst[j] = c == 1 ? img[i + j]
                            : (uint8_t)((1868 * img[3 * (i + j)] + 9617 * img[3 * (i + j) + 1] + 4899 * img[3 * (i + j) + 2] + 8192) >> 14);
    }
}

// cv::resize(level l - 1 -> level l, INTER_LINEAR), one thread per destination pixel (oracle: orc_resize_linear).  The
// source column / row and the 11-bit weights of a destination column / row depend on the level sizes only: a table made at
// creation (cv_resize_tables, the same individually rounded operations on the host) instead of two double-precision
// divisions per pixel.  Entry: x = first source index | second << 16, y = first weight | second << 16.
__global__ __launch_bounds__(256) void cv_resize_kernel(CvLevels L, int l, const int2 *__restrict__ tab, uint8_t *__restrict__ levels)
{
    const int dx = blockIdx.x * blockDim.x + threadIdx.x, dy = blockIdx.y;
    const int dw = L.w[l], sw = L.w[l - 1];
    if (dx >= dw)
        return;
    uint8_t *__restrict__ base = levels + (size_t)blockIdx.z * L.pix_total;
    const uint8_t *__restrict__ src = base + L.pix_off[l - 1];
    const int2 tx = tab[L.rs_x[l] + dx], ty = tab[L.rs_y[l] + dy];
    const int sx = tx.x & 0xffff, sx1 = tx.x >> 16, a0 = tx.y & 0xffff, a1 = tx.y >> 16;
    const int y0 = ty.x & 0xffff, y1 = ty.x >> 16, b0 = ty.y & 0xffff, b1 = ty.y >> 16;
    const uint8_t *r0 = src + (size_t)y0 * sw, *r1 = src + (size_t)y1 * sw;
    const int S0 = r0[sx] * a0 + r0[sx1] * a1, S1 = r1[sx] * a0 + r1[sx1] * a1;
    base[L.pix_off[l] + (size_t)dy * dw + dx] = (uint8_t)((((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2);
}

// The same, four destination pixels per thread: a thread's source pixels lie within eight bytes of the first one's column
// for a level ratio up to 2 (floor(a + 3 s) - floor(a) <= ceil(3 s), plus the right neighbour), so each of the two source
// rows is two dword loads and the result one dword store -- the byte-per-lane form above is bound by the number of memory
// instructions (seven per pixel), not by arithmetic.
__global__ __launch_bounds__(256) void cv_resize4_kernel(CvLevels L, int l, const int2 *__restrict__ tab, uint8_t *__restrict__ levels)
{
    const int dw = L.w[l], dh = L.h[l], sw = L.w[l - 1], qpr = (dw + 3) >> 2;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= qpr * dh)
        return;
    const int dy = t / qpr, dx = 4 * (t - dy * qpr);
    uint8_t *__restrict__ base = levels + (size_t)blockIdx.y * L.pix_total;
    const uint8_t *__restrict__ src = base + L.pix_off[l - 1];
    const int2 ty = tab[L.rs_y[l] + dy];
    const int y0 = ty.x & 0xffff, y1 = ty.x >> 16, b0 = ty.y & 0xffff, b1 = ty.y >> 16;
    int2 tx[4];
#pragma unroll
    for (int j = 0; j < 4; j++)
        tx[j] = tab[L.rs_x[l] + min(dx + j, dw - 1)];
    const int s0 = tx[0].x & 0xffff;
    unsigned lo, hi;
    __builtin_memcpy(&lo, src + (size_t)y0 * sw + s0, 4);
    __builtin_memcpy(&hi, src + (size_t)y0 * sw + s0 + 4, 4);
    const unsigned long long w0 = (unsigned long long)lo | (unsigned long long)hi << 32;
    __builtin_memcpy(&lo, src + (size_t)y1 * sw + s0, 4);
    __builtin_memcpy(&hi, src + (size_t)y1 * sw + s0 + 4, 4);
    const unsigned long long w1 = (unsigned long long)lo | (unsigned long long)hi << 32;
    unsigned out = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int c0 = 8 * ((tx[j].x & 0xffff) - s0), c1 = 8 * ((tx[j].x >> 16) - s0), a0 = tx[j].y & 0xffff, a1 = tx[j].y >> 16;
        const int S0 = (int)((w0 >> c0) & 0xffu) * a0 + (int)((w0 >> c1) & 0xffu) * a1;
        const int S1 = (int)((w1 >> c0) & 0xffu) * a0 + (int)((w1 >> c1) & 0xffu) * a1;
        out |= (unsigned)((((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2 & 0xff) << (8 * j);
    }
    uint8_t *dst = base + L.pix_off[l] + (size_t)dy * dw + dx;
    if (dx + 3 < dw) {
        __builtin_memcpy(dst, &out, 4);
    } else {
        for (int j = 0; dx + j < dw; j++)
            dst[j] = (uint8_t)(out >> (8 * j));
    }
}

// the table of level l (dw + dh entries), on the host: what the kernel used to compute per pixel, operation for operation
void cv_resize_tables(int dw, int dh, int sw, int sh, int2 *tx, int2 *ty)
{
    const double scale_x = 1. / ((double)dw / sw), scale_y = 1. / ((double)dh / sh);
    for (int dx = 0; dx < dw; dx++) {
        float fx = (float)((dx + 0.5) * scale_x - 0.5);
        int sx = (int)floorf(fx);
        fx -= sx;
        if (sx < 0)
            fx = 0, sx = 0;
        if (sx >= sw - 1)
            fx = 0, sx = sw - 1;
        const int a0 = (short)lrintf((1.f - fx) * 2048.f), a1 = (short)lrintf(fx * 2048.f);
        const int sx1 = sx + 1 < sw - 1 ? sx + 1 : sw - 1;
        tx[dx] = make_int2(sx | sx1 << 16, (a0 & 0xffff) | a1 << 16);
    }
    for (int dy = 0; dy < dh; dy++) {
        float fy = (float)((dy + 0.5) * scale_y - 0.5);
        const int sy = (int)floorf(fy);
        fy -= sy;
        const int b0 = (short)lrintf((1.f - fy) * 2048.f), b1 = (short)lrintf(fy * 2048.f);
        const int y0 = sy < 0 ? 0 : (sy > sh - 1 ? sh - 1 : sy), y1 = sy + 1 < 0 ? 0 : (sy + 1 > sh - 1 ? sh - 1 : sy + 1);
        ty[dy] = make_int2(y0 | y1 << 16, (b0 & 0xffff) | b1 << 16);
    }
}

// Gaussian 7x7 (kernel 18 34 49 55 49 34 18 in both directions, exact sums, (s + 2^15) >> 16, saturated), the FAST corner
// score and FAST's 3x3 suppression of every level of every image.  blockIdx.y = image * n_lev + level, blockIdx.x = tile.
//
// A workgroup owns a 128 x 16 tile: the 136 x 24 neighbourhood (4 rows / 4 columns of halo, reflected at the borders as
// BORDER_REFLECT_101 does) is staged in LDS once -- the thread-per-pixel form of this kernel fetched 65 bytes per pixel
// through the texture path and was 40 % of the extractor.  Then, in phases between workgroup barriers:
//   1. the horizontal 7-tap sums of 22 rows (<= 255 * 257 = 65535: a uint16, exact) go to LDS, the vertical pass reads seven
//      of them per pixel (runs of four pixels, one dword, per thread);
//   2. corners by elimination: a pre-test on every pixel of the tile and of one pixel around it (opposite ring pixels), the
//      full sixteen-pixel test on the queued eighth that passes, the score (sixteen 9-arcs, min / max chains) on the queued
//      corners -- each densely from its queue instead of by every wavefront that holds one candidate;
//   3. the suppression on the LDS score tile (the one-pixel halo holds the neighbours' scores), the survivors appended to the
//      level's candidate list.
// Scores exist inside the band the suppression reads (from one pixel outside the 31-pixel key point margin) only.
constexpr int BS_TW = 128, BS_TH = 16, BS_Q = BS_TW / 4;
constexpr int BS_SR = BS_TH + 8;              // staged rows: image rows y0 - 4 ... y0 + 19 (the ring of the score halo)
constexpr int BS_HR = BS_TH + 6;              // rows with horizontal sums: y0 - 3 ... y0 + 18
constexpr int BS_SW = BS_TW / 4 + 2;          // staged dwords per row: pixels x0 - 4 ... x0 + 131
constexpr int BS_SROW = BS_SW + 1;            // row stride in dwords
constexpr int BS_EW = BS_SW * 4, BS_ER = BS_TH + 2;   // the score tile: 136 columns (as staged) x rows y0 - 1 ... y0 + 16
constexpr int BS_BAND = CV_EDGE - 1;
constexpr int BS_KEEP = BS_TW * BS_TH / 4 + 64;       // the 3x3 suppression leaves at most one corner per 2x2

__device__ __forceinline__ int refl101_clamped(int p, int len)
{
    p = p < 0 ? -p : p;
    p = p >= len ? 2 * (len - 1) - p : p;
    return min(max(p, 0), len - 1);   // positions more than a fold outside are never read back: any valid address
}

// byte i (0 .. 11) of three consecutive dwords
__device__ __forceinline__ int byte12(unsigned d0, unsigned d1, unsigned d2, int i)
{
    return (int)(((i < 4 ? d0 : (i < 8 ? d1 : d2)) >> (8 * (i & 3))) & 0xffu);
}

__device__ __forceinline__ bool nine_of_sixteen(unsigned m)
{
    const unsigned d = m | (m << 16);
    const unsigned r2 = d & (d >> 1), r4 = r2 & (r2 >> 2), r8 = r4 & (r4 >> 4);
    return ((r8 & (d >> 8)) & 0xffffu) != 0;   // a run of eight followed by a ninth
}

__global__ __launch_bounds__(256) void cv_blur_corners_kernel(CvLevels L, int t, const uint8_t *__restrict__ levels,
                                                              uint8_t *__restrict__ blur_all, int *__restrict__ cand_count_all,
                                                              int *__restrict__ cand_idx_all, int *__restrict__ cand_score_all)
{
    __shared__ unsigned s_src[BS_SR * BS_SROW];
    __shared__ unsigned s_hs[BS_HR * BS_Q * 2];
    __shared__ unsigned s_score[BS_ER * BS_SW];          // bytes: (row, column) of the extended tile
    __shared__ unsigned short s_cand[BS_ER * BS_EW], s_queue[BS_ER * BS_EW], s_keep[BS_KEEP];
    __shared__ int s_cn, s_qn, s_kn, s_kbase;
    const int im = blockIdx.y / L.n_lev, l = blockIdx.y % L.n_lev;
    const int w = L.w[l], h = L.h[l];
    const int tiles_x = (w + BS_TW - 1) / BS_TW, tiles_y = (h + BS_TH - 1) / BS_TH;
    if (!L.on[l] || (int)blockIdx.x >= tiles_x * tiles_y)
        return;
    const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
    const int x0 = tile_x * BS_TW, y0 = tile_y * BS_TH;
    const size_t off = (size_t)im * L.pix_total + L.pix_off[l];
    const uint8_t *__restrict__ g = levels + off;
    const int tid = threadIdx.x, tx = tid & (BS_Q - 1), ty = tid >> 5;
    constexpr int CX[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
    constexpr int CY[16] = {-3, -3, -2, -1, 0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3};

    // ---- 0. the neighbourhood: rows y0 - 4 ..., columns x0 - 4 ... (dword k of a row = pixels x0 - 4 + 4k ...) ----
    const bool interior = x0 >= 4 && x0 + BS_TW + 4 <= w && y0 >= 4 && y0 + BS_TH + 4 <= h;
    for (int k = tid; k < BS_SR * BS_SW; k += 256) {
        const int r = k / BS_SW, i = k - r * BS_SW;
        const int gy = y0 - 4 + r, gx = x0 - 4 + 4 * i;
        unsigned v;
        if (interior) {
            __builtin_memcpy(&v, g + (size_t)gy * w + gx, 4);   // rows are unpadded: an unaligned dword load
        } else {
            const uint8_t *row = g + (size_t)refl101_clamped(gy, h) * w;
            v = (unsigned)row[refl101_clamped(gx, w)] | (unsigned)row[refl101_clamped(gx + 1, w)] << 8 |
                (unsigned)row[refl101_clamped(gx + 2, w)] << 16 | (unsigned)row[refl101_clamped(gx + 3, w)] << 24;
        }
        s_src[r * BS_SROW + i] = v;
    }
    for (int k = tid; k < BS_ER * BS_SW; k += 256)
        s_score[k] = 0;
    if (tid == 0) {
        s_cn = 0;
        s_qn = 0;
        s_kn = 0;
    }
    __syncthreads();

    // ---- 1a. horizontal sums of the rows y0 - 3 ... y0 + 18 (staged rows 1 ... 22) ----
    for (int k = tid; k < BS_HR * BS_Q; k += 256) {
        const int r = k / BS_Q, q = k - r * BS_Q;
        const unsigned *s = s_src + (r + 1) * BS_SROW + q;
        const unsigned d0 = s[0], d1 = s[1], d2 = s[2];
        unsigned hs[4];
#pragma unroll
        for (int j = 0; j < 4; j++)   // pixel j of the run is byte 4 + j
            hs[j] = 18u * (unsigned)(byte12(d0, d1, d2, j + 1) + byte12(d0, d1, d2, j + 7)) +
                    34u * (unsigned)(byte12(d0, d1, d2, j + 2) + byte12(d0, d1, d2, j + 6)) +
                    49u * (unsigned)(byte12(d0, d1, d2, j + 3) + byte12(d0, d1, d2, j + 5)) + 55u * (unsigned)byte12(d0, d1, d2, j + 4);
        s_hs[2 * k] = hs[0] | hs[1] << 16;
        s_hs[2 * k + 1] = hs[2] | hs[3] << 16;
    }
    // ---- 1b. a PRE-TEST of the tile and one pixel around it (the suppression's neighbours): runs of four by (row -1 ... 16,
    // dword column 0 ... 33); of the two outer columns only the pixel next to the tile is needed.  An arc of nine ring pixels
    // holds one of every two opposite ones, so a corner has, of the pairs (top, bottom) and (right, left), one brighter each
    // or one darker each: eight compares per pixel, their results combined as wave masks on the scalar unit, rows y - 3, y,
    // y + 3 only.  One pixel in eight passes on the benchmark stream (3.5 % are corners); those are queued and get the
    // full sixteen-pixel test densely (step 1c) -- every pixel through the full test was half of this kernel's instructions. ----
    for (int task = tid; task < BS_ER * BS_SW; task += 256) {
        const int er = task / BS_SW, qc = task - er * BS_SW;       // extended row 0 ... 17 = image row y0 - 1 + er
        const int y = y0 - 1 + er, x = x0 - 4 + 4 * qc;
        const unsigned jmask = qc == 0 ? 8u : (qc == BS_SW - 1 ? 1u : 15u);
        if (y < BS_BAND || y >= h - BS_BAND || x + 3 < BS_BAND || x >= w - BS_BAND)
            continue;
        const int c0 = max(qc - 1, 0), c2 = min(qc + 1, BS_SW - 1);   // a clamped dword is never one the run's ring reads
        const unsigned *rt = s_src + er * BS_SROW, *rc = rt + 3 * BS_SROW, *rb = rt + 6 * BS_SROW;   // image rows y - 3, y, y + 3
        const unsigned top = rt[qc], bot = rb[qc], m0 = rc[c0], m1 = rc[qc], m2 = rc[c2];
        unsigned cand = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int v = (int)((m1 >> (8 * j)) & 0xffu), hi = v + t, lo = v - t;
            const int pt = (int)((top >> (8 * j)) & 0xffu), pb = (int)((bot >> (8 * j)) & 0xffu);
            const int pr = byte12(m0, m1, m2, 4 + j + 3), pl = byte12(m0, m1, m2, 4 + j - 3);
            const bool pass = ((pt > hi || pb > hi) && (pr > hi || pl > hi)) || ((pt < lo || pb < lo) && (pr < lo || pl < lo));
            if (pass && ((jmask >> j) & 1u) && x + j >= BS_BAND && x + j < w - BS_BAND)
                cand |= 1u << j;
        }
        if (cand) {
            int at = atomicAdd(&s_cn, __popc(cand));
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (cand >> j & 1u)
                    s_cand[at++] = (unsigned short)(er * BS_EW + 4 * qc + j);
        }
    }
    __syncthreads();
    // ---- 1c. the full ring test of the queued pixels: sixteen differences, two 16-bit masks, a run of nine in either ----
    const uint8_t *sb = reinterpret_cast<const uint8_t *>(s_src);
    const int cn = s_cn;
    for (int e = tid; e < cn; e += 256) {
        const int pos = s_cand[e], er = pos / BS_EW, ec = pos - er * BS_EW;
        const uint8_t *c = sb + (er + 3) * (BS_SROW * 4) + ec;   // image row y0 - 1 + er is staged row er + 3
        const int v = c[0], hi = v + t, lo = v - t;
        unsigned br = 0, dk = 0;
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const int q = c[CY[k] * (BS_SROW * 4) + CX[k]];
            br |= (q > hi ? 1u : 0u) << k;
            dk |= (q < lo ? 1u : 0u) << k;
        }
        if (nine_of_sixteen(br) || nine_of_sixteen(dk))
            s_queue[atomicAdd(&s_qn, 1)] = (unsigned short)pos;
    }
    __syncthreads();

    // ---- 2a. vertical sums -> the blurred level ----
#pragma unroll
    for (int half = 0; half < 2; half++) {
        const int oy = ty + 8 * half, y = y0 + oy, x = x0 + 4 * tx;
        constexpr unsigned K[7] = {18, 34, 49, 55, 49, 34, 18};
        unsigned s0 = 0, s1 = 0, s2 = 0, s3 = 0;
#pragma unroll
        for (int r = 0; r < 7; r++) {
            const unsigned a = s_hs[2 * ((oy + r) * BS_Q + tx)], b = s_hs[2 * ((oy + r) * BS_Q + tx) + 1];
            s0 += K[r] * (a & 0xffffu);
            s1 += K[r] * (a >> 16);
            s2 += K[r] * (b & 0xffffu);
            s3 += K[r] * (b >> 16);
        }
        const unsigned o0 = min((s0 + (1u << 15)) >> 16, 255u), o1 = min((s1 + (1u << 15)) >> 16, 255u),
                       o2 = min((s2 + (1u << 15)) >> 16, 255u), o3 = min((s3 + (1u << 15)) >> 16, 255u);
        const unsigned packed = o0 | o1 << 8 | o2 << 16 | o3 << 24;
        if (y < h && x < w) {
            uint8_t *dst = blur_all + off + (size_t)y * w + x;
            if (x + 3 < w) {
                __builtin_memcpy(dst, &packed, 4);
            } else {
                for (int j = 0; x + j < w; j++)
                    dst[j] = (uint8_t)(packed >> (8 * j));
            }
        }
    }
    // ---- 2b. cornerScore<16> of the queued pixels: max over the sixteen 9-arcs of min(d) / of min(-d), at least t ----
    const int qn = s_qn;
    uint8_t *sc = reinterpret_cast<uint8_t *>(s_score);
    for (int e = tid; e < qn; e += 256) {
        const int pos = s_queue[e], er = pos / BS_EW, ec = pos - er * BS_EW;
        const uint8_t *c = sb + (er + 3) * (BS_SROW * 4) + ec;   // image row y0 - 1 + er is staged row er + 3
        const int v = c[0];
        int d[16];
#pragma unroll
        for (int k = 0; k < 16; k++)
            d[k] = v - (int)c[CY[k] * (BS_SROW * 4) + CX[k]];
        int a0 = t, b0;
#pragma unroll
        for (int k = 0; k < 16; k += 2) {
            int a = min(d[(k + 1) & 15], d[(k + 2) & 15]);
#pragma unroll
            for (int i = 3; i <= 8; i++)
                a = min(a, d[(k + i) & 15]);
            a0 = max(a0, min(a, d[k]));
            a0 = max(a0, min(a, d[(k + 9) & 15]));
        }
        b0 = -a0;
#pragma unroll
        for (int k = 0; k < 16; k += 2) {
            int b = max(d[(k + 1) & 15], d[(k + 2) & 15]);
#pragma unroll
            for (int i = 3; i <= 8; i++)
                b = max(b, d[(k + i) & 15]);
            b0 = min(b0, max(b, d[k]));
            b0 = min(b0, max(b, d[(k + 9) & 15]));
        }
        sc[pos] = (uint8_t)(-b0 - 1);
    }
    __syncthreads();

    // ---- 3. FAST's 3x3 suppression (strictly above all eight neighbours' scores) of the tile's own corners inside the
    // 31-pixel key point margin; the survivors are this tile's candidates ----
    for (int e = tid; e < qn; e += 256) {
        const int pos = s_queue[e], er = pos / BS_EW, ec = pos - er * BS_EW;
        const int x = x0 - 4 + ec, y = y0 - 1 + er;
        if (er < 1 || er > BS_TH || ec < 4 || ec >= 4 + BS_TW || x < CV_EDGE || x >= w - CV_EDGE || y < CV_EDGE || y >= h - CV_EDGE)
            continue;
        const uint8_t *p = sc + pos;
        const int s = p[0];
        const int top = max(max(max(p[-1], p[1]), max(p[-BS_EW - 1], p[-BS_EW])), max(max(p[-BS_EW + 1], p[BS_EW - 1]), max(p[BS_EW], p[BS_EW + 1])));
        if (s > top) {
            const int at = atomicAdd(&s_kn, 1);
            if (at < BS_KEEP)
                s_keep[at] = (unsigned short)pos;
        }
    }
    __syncthreads();
    // ---- 4. appended to the level's candidate list (any order: cv_select_kernel ranks by pixel index where order matters) ----
    const int kn = min(s_kn, BS_KEEP);
    if (tid == 0 && kn > 0)
        s_kbase = atomicAdd(cand_count_all + blockIdx.y, kn);
    __syncthreads();
    if (kn > 0) {
        const int cap = L.cand_cap[l];
        const size_t coff = (size_t)im * L.cand_total + L.cand_off[l];
        for (int e = tid; e < kn; e += 256) {
            const int pos = s_keep[e], er = pos / BS_EW, ec = pos - er * BS_EW;
            const int at = s_kbase + e;
            if (at < cap) {
                cand_idx_all[coff + at] = (y0 - 1 + er) * w + (x0 - 4 + ec);
                cand_score_all[coff + at] = sc[pos];
            }
        }
    }
}

__device__ __forceinline__ unsigned sortable_key(float f)
{
    const unsigned b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// the response from the window's three integer sums (upstream's HarrisResponses: k = 0.04, scale 1 / (4 * 7 * 255) to the fourth)
__device__ __forceinline__ float harris_of(int a, int b, int c)
{
    const float fa = (float)a, fb = (float)b, fc = (float)c;
    const float sc = 1.f / (4 * 7 * 255.f);
    const float s4 = sc * sc * sc * sc;
    return (fa * fb - fc * fc - 0.04f * (fa + fb) * (fa + fb)) * s4;
}

__device__ __forceinline__ float harris_at(const uint8_t *__restrict__ g, int w, int x, int y)
{
    int a = 0, b = 0, c = 0;
    const uint8_t *p0 = g + (size_t)y * w + x;
    for (int j = -3; j <= 3; j++) {
        const uint8_t *r = p0 + (ptrdiff_t)j * w;
#pragma unroll
        for (int i = -3; i <= 3; i++) {
            const uint8_t *q = r + i;
            const int ix = (q[1] - q[-1]) * 2 + (q[-w + 1] - q[-w - 1]) + (q[w + 1] - q[w - 1]);
            const int iy = (q[w] - q[-w]) * 2 + (q[w - 1] - q[-w - 1]) + (q[w + 1] - q[-w + 1]);
            a += ix * ix;
            b += iy * iy;
            c += ix * iy;
        }
    }
    return harris_of(a, b, c);
}

// One workgroup per (image, level): retainBest(2 want) by the FAST score (ties kept), Harris of the survivors,
// retainBest(want) by it (ties at the cut: raster-earlier first), written in raster order -- whatever order the candidates
// come in.
// 1024 threads: the survivors' Harris responses (49 x 8 byte loads each) are this kernel's longest stretch, and they spread over
// the threads -- 51 us per 16 images against 106 with 256 threads (tried for the sake of the beside-the-tracker rule of
// beside the front-end the detector's time is the same either way, alone it is the shorter chain that
// counts).
constexpr int CV_SEL_T = 1024;
constexpr int CV_SEL_KEEP = 2048;   // the largest per-level quota a selection holds (svo_orb_cv_create checks)
constexpr int CV_SEL_SURV = 1024;   // survivors of the FAST cut whose Harris windows are dealt out row by row; more: a thread each
constexpr int CV_SEL_TIES = 1024;   // ties at the cut listed in LDS; beyond: ranked against the candidate list itself
__global__ __launch_bounds__(CV_SEL_T) void cv_select_kernel(CvLevels L, const uint8_t *__restrict__ levels,
                                                         const int *__restrict__ cand_idx_all, const int *__restrict__ cand_score_all,
                                                         float *__restrict__ cand_resp_all, const int *__restrict__ d_nc_all,
                                                         int *__restrict__ sel_idx_all, float *__restrict__ sel_resp_all,
                                                         int *__restrict__ d_nsel_all)
{
    __shared__ int s_red[CV_SEL_T / 64], s_base, s_ties, s_hist[256], s_pick, s_left, s_nk;
    __shared__ int s_tie[CV_SEL_TIES], s_kidx[CV_SEL_KEEP], s_spos[CV_SEL_SURV], s_abc[3 * CV_SEL_SURV];
    __shared__ float s_kresp[CV_SEL_KEEP];
    const int im = blockIdx.x / L.n_lev, l = blockIdx.x % L.n_lev;
    const int cap = L.cand_cap[l], want = L.want[l], w = L.w[l];
    const size_t coff = (size_t)im * L.cand_total + L.cand_off[l];
    const int *__restrict__ cand_idx = cand_idx_all + coff;
    const int *__restrict__ cand_score = cand_score_all + coff;
    float *__restrict__ cand_resp = cand_resp_all + coff;
    int *__restrict__ sel_idx = sel_idx_all + ((size_t)im * L.n_lev + l) * L.n_features;
    float *__restrict__ sel_resp = sel_resp_all + ((size_t)im * L.n_lev + l) * L.n_features;
    int *__restrict__ d_nsel = d_nsel_all + blockIdx.x;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (!L.on[l] || want <= 0) {
        if (t == 0)
            *d_nsel = 0;
        return;
    }
    const uint8_t *__restrict__ g = levels + (size_t)im * L.pix_total + L.pix_off[l];
    const int nc = min(d_nc_all[blockIdx.x], cap);
    // ---- the FAST-score cut: the largest `cut` with count(score >= cut) >= 2 want; everything when nc <= 2 want ----
    if (t < 256)
        s_hist[t] = 0;
    if (t == 0)
        s_nk = 0;
    __syncthreads();
    for (int i = t; i < nc; i += CV_SEL_T)
        atomicAdd(&s_hist[cand_score[i] & 255], 1);
    __syncthreads();
    int cut = 0;
    if (nc > 2 * want) {
        // a suffix sum over the bins by 256 threads: above[t] = candidates with a score over t
        int cnt = 0, incl = 0;
        if (t < 256) {
            cnt = s_hist[t];
            incl = cnt;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int o = __shfl_down(incl, off, 64);
                incl += lane + off < 64 ? o : 0;
            }
            if (lane == 0)
                s_red[wave] = incl;
        }
        __syncthreads();
        if (t < 256) {
            int above = incl - cnt;
            for (int w2 = wave + 1; w2 < 4; w2++)
                above += s_red[w2];
            if (above < 2 * want && 2 * want <= above + cnt)
                s_pick = t;
        }
        __syncthreads();
        cut = s_pick;
        __syncthreads();
    }
    // ---- Harris response of the survivors; the others get the lowest key.  The survivors are listed in LDS and their 7 x 7
    // windows dealt out ROW BY ROW (seven tasks per survivor over all the threads; the integer sums of a window meet in LDS
    // atomics, exact in any order): a thread per survivor walking 49 x 8 bytes alone was this kernel's longest stretch. ----
    for (int i = t; i < nc; i += CV_SEL_T) {
        const bool in = cand_score[i] >= cut;
        if (in) {
            const int at = atomicAdd(&s_nk, 1);
            if (at < CV_SEL_SURV) {
                s_spos[at] = i;
                s_abc[3 * at] = s_abc[3 * at + 1] = s_abc[3 * at + 2] = 0;
            }
        } else {
            cand_resp[i] = -INFINITY;
        }
    }
    __syncthreads();
    const int nk = s_nk;
    if (nk <= CV_SEL_SURV) {
        for (int task = t; task < nk * 7; task += CV_SEL_T) {
            const int a = task / 7, j = task - 7 * a - 3;
            const int idx = cand_idx[s_spos[a]];
            const int y = idx / w, x = idx - y * w;
            const uint8_t *r = g + (size_t)(y + j) * w + x;
            int sa = 0, sb = 0, sc2 = 0;
#pragma unroll
            for (int i = -3; i <= 3; i++) {
                const uint8_t *q = r + i;
                const int ix = (q[1] - q[-1]) * 2 + (q[-w + 1] - q[-w - 1]) + (q[w + 1] - q[w - 1]);
                const int iy = (q[w] - q[-w]) * 2 + (q[w - 1] - q[-w - 1]) + (q[w + 1] - q[-w + 1]);
                sa += ix * ix;
                sb += iy * iy;
                sc2 += ix * iy;
            }
            atomicAdd(&s_abc[3 * a], sa);
            atomicAdd(&s_abc[3 * a + 1], sb);
            atomicAdd(&s_abc[3 * a + 2], sc2);
        }
        __syncthreads();
        for (int a = t; a < nk; a += CV_SEL_T)
            cand_resp[s_spos[a]] = harris_of(s_abc[3 * a], s_abc[3 * a + 1], s_abc[3 * a + 2]);
    } else {   // more survivors than the list holds (a level of ties at the FAST cut): a thread per survivor
        for (int i = t; i < nc; i += CV_SEL_T)
            if (cand_score[i] >= cut) {
                const int idx = cand_idx[i];
                cand_resp[i] = harris_at(g, w, idx % w, idx / w);
            }
    }
    __syncthreads();
    // ---- the want-th largest response among the nk survivors, a byte at a time (orb.hip's select) ----
    unsigned thr = 0;
    int n_above = 0;
    if (nk > want) {
        int left = want;
        for (int shift = 24; shift >= 0; shift -= 8) {
            if (t < 256)
                s_hist[t] = 0;
            __syncthreads();
            const unsigned himask = shift == 24 ? 0u : 0xffffffffu << (shift + 8);
            for (int i = t; i < nc; i += CV_SEL_T) {
                const unsigned k = sortable_key(cand_resp[i]);
                if ((k & himask) == (thr & himask))
                    atomicAdd(&s_hist[(k >> shift) & 255u], 1);
            }
            __syncthreads();
            int cnt = 0, incl = 0;
            if (t < 256) {
                cnt = s_hist[t];
                incl = cnt;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const int o = __shfl_down(incl, off, 64);
                    incl += lane + off < 64 ? o : 0;
                }
                if (lane == 0)
                    s_red[wave] = incl;
            }
            __syncthreads();
            if (t < 256) {
                int above = incl - cnt;
                for (int w2 = wave + 1; w2 < 4; w2++)
                    above += s_red[w2];
                if (above < left && left <= above + cnt) {
                    s_pick = t;
                    s_left = left - above;
                }
            }
            __syncthreads();
            thr |= (unsigned)s_pick << shift;
            left = s_left;
            __syncthreads();
        }
        n_above = want - left;
    }
    // ---- the kept ones, in raster order.  The candidate list comes in ANY order (the tiles of cv_blur_corners_kernel append
    // as they finish), so order is made here from the pixel index: the ties at the cut that stay are the `ties_allowed`
    // with the smallest index, and a kept candidate's place is the number of kept ones with a smaller index. ----
    const unsigned lowest = sortable_key(-INFINITY);   // a candidate below the FAST cut
    const int ties_allowed = nk > want ? want - n_above : 0;
    if (t == 0) {
        s_base = 0;   // kept so far
        s_ties = 0;   // ties listed
    }
    __syncthreads();
    for (int i = t; i < nc; i += CV_SEL_T) {   // the ties' pixel indices (their number is usually one: the cut itself)
        if (nk > want && sortable_key(cand_resp[i]) == thr) {
            const int at = atomicAdd(&s_ties, 1);
            if (at < CV_SEL_TIES)
                s_tie[at] = cand_idx[i];
        }
    }
    __syncthreads();
    const int nt = s_ties;
    for (int i = t; i < nc; i += CV_SEL_T) {
        const unsigned key = sortable_key(cand_resp[i]);
        if (key == lowest)
            continue;
        bool keep = nk <= want || key > thr;
        if (!keep && key == thr && ties_allowed > 0) {
            const int idx = cand_idx[i];
            int rank = 0;
            if (nt <= CV_SEL_TIES) {
                for (int k = 0; k < nt; k++)
                    rank += s_tie[k] < idx ? 1 : 0;
            } else {   // more ties than the list holds (a level of repeating texture): against the candidates themselves
                for (int k = 0; k < nc; k++)
                    rank += (sortable_key(cand_resp[k]) == thr && cand_idx[k] < idx) ? 1 : 0;
            }
            keep = rank < ties_allowed;
        }
        if (keep) {
            const int at = atomicAdd(&s_base, 1);
            if (at < CV_SEL_KEEP) {
                s_kidx[at] = cand_idx[i];
                s_kresp[at] = cand_resp[i];
            }
        }
    }
    __syncthreads();
    const int kept = min(s_base, CV_SEL_KEEP);
    for (int a = t; a < kept; a += CV_SEL_T) {
        const int idx = s_kidx[a];
        int pos = 0;
        for (int k = 0; k < kept; k++)
            pos += s_kidx[k] < idx ? 1 : 0;
        sel_idx[pos] = idx;
        sel_resp[pos] = s_kresp[a];
    }
    if (t == 0)
        *d_nsel = kept;
}

// one wavefront per selected key point; grid (ceil(max want / 4), n_lev, batch)
__global__ __launch_bounds__(256) void cv_describe_kernel(CvLevels L, const uint8_t *__restrict__ levels,
                                                          const uint8_t *__restrict__ blur_all, const int *__restrict__ sel_idx_all,
                                                          const float *__restrict__ sel_resp_all, const int *__restrict__ d_nsel_all,
                                                          const int8_t *__restrict__ pat, int cap_out, int *__restrict__ d_total,
                                                          float *__restrict__ xy, int *__restrict__ oct, float *__restrict__ resp,
                                                          float *__restrict__ dir, uint32_t *__restrict__ desc)
{
    const int lane = threadIdx.x & 63, l = blockIdx.y, im = blockIdx.z;
    const int *__restrict__ nsel = d_nsel_all + (size_t)im * L.n_lev;
    int out_base = 0, total = 0;
    for (int q = 0; q < L.n_lev; q++) {
        const int nq = nsel[q];
        out_base += q < l ? nq : 0;
        total += nq;
    }
    if (blockIdx.x == 0 && l == 0 && threadIdx.x == 0)
        d_total[im] = min(total, cap_out);
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= nsel[l] || out_base + i >= cap_out)
        return;
    const int w = L.w[l];
    const size_t off = (size_t)im * L.pix_total + L.pix_off[l];
    const uint8_t *__restrict__ g = levels + off;
    const uint8_t *__restrict__ blur = blur_all + off;
    const size_t sbase = ((size_t)im * L.n_lev + l) * L.n_features;
    const int idx = sel_idx_all[sbase + i], x = idx % w, y = idx / w;
    // the 31-pixel disc with upstream's umax table, row by row
    int m10 = 0, m01 = 0;
    for (int e = lane; e < 31 * 31; e += 64) {
        const int v = e / 31 - 15, u = e % 31 - 15;
        constexpr int UMAX[16] = {15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3};
        const int av = v < 0 ? -v : v, au = u < 0 ? -u : u;
        // UMAX as a compare chain (a constant table indexed per lane would live in scratch)
        int um = 3;
        um = av <= 14 ? 6 : um;
        um = av <= 13 ? 8 : um;
        um = av <= 12 ? 9 : um;
        um = av <= 11 ? 10 : um;
        um = av <= 10 ? 11 : um;
        um = av <= 9 ? 12 : um;
        um = av <= 8 ? 13 : um;
        um = av <= 6 ? 14 : um;
        um = av <= 3 ? 15 : um;
        (void)UMAX;
        if (au <= um) {
            const int p = g[(ptrdiff_t)(y + v) * w + x + u];
            m10 += u * p;
            m01 += v * p;
        }
    }
    m10 = svo::wave_sum(m10);
    m01 = svo::wave_sum(m01);
    const float ang = fast_atan2_deg((float)m01, (float)m10);
    const float rad = ang * (float)(3.14159265358979323846 / 180.f);
    const float a = (float)svo_cos((double)rad), b = (float)svo_sin((double)rad);
    const size_t o = (size_t)im * cap_out + out_base + i;
    uint32_t *d = desc + 8 * o;
    const uint8_t *bc = blur + (size_t)y * w + x;
#pragma unroll
    for (int pass = 0; pass < 4; pass++) {
        const int tt = pass * 64 + lane;
        const int px1 = pat[4 * tt], py1 = pat[4 * tt + 1], px2 = pat[4 * tt + 2], py2 = pat[4 * tt + 3];
        const float x1 = px1 * a - py1 * b, y1 = px1 * b + py1 * a;
        const float x2 = px2 * a - py2 * b, y2 = px2 * b + py2 * a;
        const int t0 = bc[__float2int_rn(y1) * w + __float2int_rn(x1)], t1 = bc[__float2int_rn(y2) * w + __float2int_rn(x2)];
        const unsigned long long bits = __ballot(t0 < t1);
        if (lane == 0) {
            d[2 * pass] = (uint32_t)bits;
            d[2 * pass + 1] = (uint32_t)(bits >> 32);
        }
    }
    if (lane == 0) {
        xy[2 * o] = (float)x * L.scale[l];
        xy[2 * o + 1] = (float)y * L.scale[l];
        oct[o] = l;
        resp[o] = sel_resp_all[sbase + i];
        dir[2 * o] = a;
        dir[2 * o + 1] = b;
    }
}

}  // namespace

struct svo_orb_cv {
    svo_ctx *ctx = nullptr;
    int w = 0, h = 0, c = 0, batch = 0, fast_t = 20;
    CvLevels lv;
    int max_want = 0;
    DevBuf levels, blur, cand_idx, cand_score, cand_resp, sel_idx, sel_resp, counts, pat, rs_tab;
};

void svo_orb_default_pattern(int8_t *pat)
{
    // the seeded generator stated in oracle/orb.c (orc_orb_pattern)
    uint32_t s = 0x9E3779B9u;
    for (int i = 0; i < 256 * 4; i++) {
        int acc = 0;
        for (int k = 0; k < 3; k++) {
            s = s * 1664525u + 1013904223u;
            acc += (int)((s >> 16) % 27u) - 13;
        }
        int v = acc / 2;
        v = v > 13 ? 13 : (v < -13 ? -13 : v);
        pat[i] = (int8_t)v;
    }
    for (int i = 0; i < 256; i++)
        if (pat[4 * i] == pat[4 * i + 2] && pat[4 * i + 1] == pat[4 * i + 3])
            pat[4 * i + 2] = (int8_t)(pat[4 * i + 2] >= 0 ? pat[4 * i + 2] - 1 : pat[4 * i + 2] + 1);
}

int svo_orb_cv_destroy(svo_orb_cv *o)
{
    if (!o)
        return SVO_OK;
    (void)hipStreamSynchronize(o->ctx->stream);
    DevBuf *bufs[] = {&o->levels, &o->blur, &o->cand_idx,
                      &o->cand_score, &o->cand_resp, &o->sel_idx, &o->sel_resp, &o->counts, &o->pat, &o->rs_tab};
    for (DevBuf *b : bufs)
        b->release();
    delete o;
    return SVO_OK;
}

int svo_orb_cv_set_pattern(svo_orb_cv *o, const int8_t *pattern)
{
    int8_t pat[1024];
    if (pattern)
        memcpy(pat, pattern, 1024);
    else
        svo_orb_default_pattern(pat);
    SVO_HIP(hipMemcpyAsync(o->pat.p, pat, sizeof(pat), hipMemcpyHostToDevice, o->ctx->stream));
    SVO_HIP(hipStreamSynchronize(o->ctx->stream));   // pat is a stack array
    return SVO_OK;
}

int svo_orb_cv_create(svo_ctx *ctx, int w, int h, int c, int n_features, int fast_t, int n_levels, float scale_factor, int batch,
                      const int8_t *pattern, svo_orb_cv **out)
{
    SVO_CHECK_ARG(ctx && out && w > 2 * CV_EDGE && h > 2 * CV_EDGE && (c == 1 || c == 3) && n_features > 0 && fast_t > 0);
    SVO_CHECK_ARG(n_levels >= 1 && n_levels <= CV_MAXLEV && scale_factor > 1.f && batch >= 1 && batch <= CV_MAXBATCH);
    svo_orb_cv *o = new svo_orb_cv();
    o->ctx = ctx;
    o->w = w;
    o->h = h;
    o->c = c;
    o->batch = batch;
    o->fast_t = fast_t;
    CvLevels &L = o->lv;
    memset(&L, 0, sizeof(L));
    L.n_lev = n_levels;
    L.n_features = n_features;
    // the levels and their quota exactly as oracle/orb.c:orc_orb_cv_levels (cv::ORB: getScale, the per-level feature split)
    for (int l = 0; l < n_levels; l++) {
        L.scale[l] = (float)pow((double)scale_factor, (double)l);
        L.w[l] = (int)lrintf((float)w / L.scale[l]);
        L.h[l] = (int)lrintf((float)h / L.scale[l]);
    }
    const float factor = (float)(1.0 / scale_factor);
    float want = n_features * (1 - factor) / (1 - (float)pow((double)factor, (double)n_levels));
    int sum = 0;
    for (int l = 0; l < n_levels - 1; l++) {
        L.want[l] = (int)lrintf(want);
        sum += L.want[l];
        want *= factor;
    }
    L.want[n_levels - 1] = n_features - sum > 0 ? n_features - sum : 0;
    size_t pix = 0, cand = 0;
    for (int l = 0; l < n_levels; l++) {
        if (L.w[l] < 8 || L.h[l] < 8) {   // the blur's reflection folds once
            L.n_lev = l;
            break;
        }
        L.on[l] = L.w[l] > 2 * CV_EDGE && L.h[l] > 2 * CV_EDGE && L.want[l] > 0;
        const size_t npix = (size_t)L.w[l] * L.h[l];
        L.pix_off[l] = (int)pix;
        L.cand_off[l] = (int)cand;
        L.cand_cap[l] = (int)(npix / 4 + 1024);   // the 3x3 suppression leaves at most one corner per 2x2
        o->max_want = L.want[l] > o->max_want ? L.want[l] : o->max_want;
        pix += (npix + 63) & ~(size_t)63;
        cand += L.cand_cap[l];
    }
    L.pix_total = (int)pix;
    L.cand_total = (int)cand;
    if (o->max_want > CV_SEL_KEEP) {
        svo_set_error("svo_orb_cv_create: a level's feature quota is %d; the selection holds at most %d (n_features too large)", o->max_want, CV_SEL_KEEP);
        svo_orb_cv_destroy(o);
        return SVO_ERR_ARG;
    }
    std::vector<int2> tab;
    for (int l = 1; l < L.n_lev; l++) {
        L.rs_x[l] = (int)tab.size();
        L.rs_y[l] = L.rs_x[l] + L.w[l];
        tab.resize(tab.size() + (size_t)L.w[l] + L.h[l]);
        cv_resize_tables(L.w[l], L.h[l], L.w[l - 1], L.h[l - 1], tab.data() + L.rs_x[l], tab.data() + L.rs_y[l]);
    }
    const size_t B = (size_t)batch;
    int rc;
    if ((rc = o->levels.ensure(B * pix + 64)) ||   // + 64: cv_resize4_kernel reads eight bytes from a row's last column
         (rc = o->blur.ensure(B * pix)) ||
        (rc = o->cand_idx.ensure(B * cand * 4)) || (rc = o->cand_score.ensure(B * cand * 4)) || (rc = o->cand_resp.ensure(B * cand * 4)) ||
        (rc = o->sel_idx.ensure(B * CV_MAXLEV * n_features * 4 + 64)) || (rc = o->sel_resp.ensure(B * CV_MAXLEV * n_features * 4 + 64)) ||
        (rc = o->counts.ensure(B * CV_MAXLEV * 2 * 4 + 64)) || (rc = o->pat.ensure(1024)) || (rc = svo_orb_cv_set_pattern(o, pattern)) ||
        (rc = o->rs_tab.ensure(tab.size() * sizeof(int2) + 64))) {
        svo_orb_cv_destroy(o);
        return rc;
    }
    if (!tab.empty()) {
        hipError_t e = hipMemcpyAsync(o->rs_tab.p, tab.data(), tab.size() * sizeof(int2), hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess)
            e = hipStreamSynchronize(ctx->stream);   // tab is a local
        if (e != hipSuccess) {
            svo_orb_cv_destroy(o);
            svo_set_error("svo_orb_cv_create: table upload -> %s", hipGetErrorString(e));
            return SVO_ERR_HIP;
        }
    }
    *out = o;
    return SVO_OK;
}

int svo_orb_cv_batch(const svo_orb_cv *o) { return o->batch; }

// n_images device images (h x w x c) -> device outputs of n_images x cap_out entries (cap_out >= 1; features beyond it are
// dropped) and d_n[n_images].  Asynchronous on `st` (NULL: the context's stream).
int svo_orb_cv_launch(svo_orb_cv *o, const uint8_t *const *d_images, int n_images, int cap_out, float *d_xy, int *d_oct,
                      float *d_resp, float *d_dir, uint32_t *d_desc, int *d_n, hipStream_t st)
{
    SVO_CHECK_ARG(o && d_images && n_images >= 1 && n_images <= o->batch && cap_out >= 1);
    if (!st)
        st = o->ctx->stream;
    const CvLevels &L = o->lv;
    CvImages im;
    memset(&im, 0, sizeof(im));
    for (int k = 0; k < n_images; k++)
        im.img[k] = d_images[k];
    const int B = n_images, npix0 = o->w * o->h;
    uint8_t *lv = o->levels.as<uint8_t>();
    hipLaunchKernelGGL(cv_gray_kernel, dim3((npix0 + 1023) / 1024, B), dim3(256), 0, st, im, npix0, o->c, lv, L.pix_total);
    for (int l = 1; l < L.n_lev; l++)
        if (L.w[l - 1] <= 2 * L.w[l]) {   // four pixels per thread: a thread's sources within eight bytes (ratio <= 2)
            const int quads = ((L.w[l] + 3) / 4) * L.h[l];
            hipLaunchKernelGGL(cv_resize4_kernel, dim3((quads + 255) / 256, B), dim3(256), 0, st, L, l, o->rs_tab.as<int2>(), lv);
        } else {
            hipLaunchKernelGGL(cv_resize_kernel, dim3((L.w[l] + 255) / 256, L.h[l], B), dim3(256), 0, st, L, l, o->rs_tab.as<int2>(), lv);
        }
    int *d_nc = o->counts.as<int>(), *d_nsel = d_nc + (size_t)o->batch * CV_MAXLEV;
    const int bs_tiles = ((L.w[0] + BS_TW - 1) / BS_TW) * ((L.h[0] + BS_TH - 1) / BS_TH);   // level 0 has the most
    // the candidate counters start from zero: the tiles of a level append their suppression's survivors to the level's list
    SVO_HIP(hipMemsetAsync(d_nc, 0, (size_t)B * L.n_lev * sizeof(int), st));
    hipLaunchKernelGGL(cv_blur_corners_kernel, dim3(bs_tiles, B * L.n_lev), dim3(256), 0, st, L, o->fast_t, lv, o->blur.as<uint8_t>(),
                       d_nc, o->cand_idx.as<int>(), o->cand_score.as<int>());
    hipLaunchKernelGGL(cv_select_kernel, dim3(B * L.n_lev), dim3(CV_SEL_T), 0, st, L, lv, o->cand_idx.as<int>(), o->cand_score.as<int>(),
                       o->cand_resp.as<float>(), d_nc, o->sel_idx.as<int>(), o->sel_resp.as<float>(), d_nsel);
    hipLaunchKernelGGL(cv_describe_kernel, dim3((o->max_want + 3) / 4, L.n_lev, B), dim3(256), 0, st, L, lv, o->blur.as<uint8_t>(),
                       o->sel_idx.as<int>(), o->sel_resp.as<float>(), d_nsel, o->pat.as<int8_t>(), cap_out, d_n, d_xy, d_oct, d_resp,
                       d_dir, d_desc);
    SVO_HIP(hipGetLastError());
    return SVO_OK;
}

extern "C" {

void svo_orb_default_params(svo_orb_params *p)
{
    if (!p)
        return;
    p->n_features = 500;   // ORB::create()
    p->fast_threshold = 20;
    p->shape = SVO_ORB_SHAPE_CV;
    p->n_levels = 8;
    p->scale_factor = 1.2f;
}

int svo_orb_set_pattern(svo_ctx *ctx, const int8_t *pattern)
{
    SVO_CHECK_ARG(ctx);
    if (pattern) {
        for (int i = 0; i < 1024; i++)
            if (pattern[i] < -15 || pattern[i] > 15) {
                svo_set_error("svo_orb_set_pattern: coordinate %d of the pattern is %d (|.| <= 15: a rotated test must stay inside "
                              "the 31-pixel margin)", i, (int)pattern[i]);
                return SVO_ERR_ARG;
            }
        memcpy(ctx->orb_pattern, pattern, 1024);
        ctx->has_pattern = 1;
    } else {
        ctx->has_pattern = 0;
    }
    SVO_HIP(hipSetDevice(ctx->device));
    if (ctx->orb_cv_cache)
        return svo_orb_cv_set_pattern(ctx->orb_cv_cache, ctx->has_pattern ? ctx->orb_pattern : nullptr);
    return SVO_OK;
}

int svo_orb_extract_batch(svo_ctx *ctx, const uint8_t *const *images, int n_images, int w, int h, int c, const svo_orb_params *prm,
                          float *xy, int *octave, float *response, float *dir, uint32_t *desc, int *n, int mem)
{
    SVO_CHECK_ARG(ctx && images && n_images >= 0 && xy && desc && n);
    SVO_CHECK_ARG(mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE);
    svo_orb_params p;
    if (prm)
        p = *prm;
    else
        svo_orb_default_params(&p);
    SVO_CHECK_ARG(p.n_features > 0 && p.fast_threshold > 0);
    const size_t nf = (size_t)p.n_features;
    if (p.shape == SVO_ORB_SHAPE_OCTAVES3) {   // the earlier rounds' shape: one image per set of launches
        for (int i = 0; i < n_images; i++) {
            const int rc = svo_orb_extract(ctx, images[i], w, h, c, p.n_features, p.fast_threshold, xy + 2 * nf * i,
                                           octave ? octave + nf * i : nullptr, response ? response + nf * i : nullptr,
                                           dir ? dir + 2 * nf * i : nullptr, desc + 8 * nf * i, n + i, mem);
            if (rc)
                return rc;
        }
        return SVO_OK;
    }
    SVO_CHECK_ARG(p.shape == SVO_ORB_SHAPE_CV);
    if (n_images == 0)
        return SVO_OK;
    SVO_HIP(hipSetDevice(ctx->device));
    const int B = n_images < CV_MAXBATCH ? n_images : CV_MAXBATCH;
    int sf_bits;
    memcpy(&sf_bits, &p.scale_factor, 4);
    const int key[8] = {w, h, c, p.n_features, p.fast_threshold, p.n_levels, sf_bits, 0};
    int rc;
    if (!ctx->orb_cv_cache || memcmp(key, ctx->orb_cv_key, sizeof(int) * 7) != 0 || svo_orb_cv_batch(ctx->orb_cv_cache) < B) {
        if (ctx->orb_cv_cache)
            svo_orb_cv_destroy(ctx->orb_cv_cache);
        ctx->orb_cv_cache = nullptr;
        if ((rc = svo_orb_cv_create(ctx, w, h, c, p.n_features, p.fast_threshold, p.n_levels, p.scale_factor, B,
                                    ctx->has_pattern ? ctx->orb_pattern : nullptr, &ctx->orb_cv_cache)))
            return rc;
        memcpy(ctx->orb_cv_key, key, sizeof(key));
    }
    svo_orb_cv *o = ctx->orb_cv_cache;
    hipStream_t st = ctx->stream;
    const size_t img_bytes = (size_t)w * h * c, rec = 8 + 4 + 4 + 8 + 32;
    DevBuf &out = ctx->orb_cv_out;
    // (device outputs: the counts of ALL the images live behind the group block, so that the groups follow each other on the
    // stream without a wait in between -- one read-back at the end)
    const size_t count_off = ((size_t)B * nf * rec + (size_t)B * 4 + 63) & ~(size_t)63;
    if ((rc = out.ensure(count_off + (size_t)n_images * 4 + 64)) || (mem == SVO_MEM_HOST && (rc = ctx->orb_cv_img.ensure((size_t)B * img_bytes))))
        return rc;
    int *dn_all = reinterpret_cast<int *>(out.as<uint8_t>() + count_off);
    std::vector<unsigned char> &hb = ctx->orb_host;
    for (int first = 0; first < n_images; first += B) {
        const int nb = n_images - first < B ? n_images - first : B;
        // the block of a group: xy | octave | response | dir | desc | n, each for nb x nf entries
        float *dxy = out.as<float>();
        int *doct = reinterpret_cast<int *>(dxy + 2 * nf * B);
        float *dresp = reinterpret_cast<float *>(doct + nf * B), *ddir = dresp + nf * B;
        uint32_t *ddesc = reinterpret_cast<uint32_t *>(ddir + 2 * nf * B);
        int *dn = reinterpret_cast<int *>(ddesc + 8 * nf * B);
        const uint8_t *ptrs[CV_MAXBATCH];
        for (int k = 0; k < nb; k++) {
            if (mem == SVO_MEM_HOST) {
                uint8_t *slot = ctx->orb_cv_img.as<uint8_t>() + (size_t)k * img_bytes;
                SVO_HIP(hipMemcpyAsync(slot, images[first + k], img_bytes, hipMemcpyHostToDevice, st));
                ptrs[k] = slot;
            } else {
                ptrs[k] = images[first + k];
            }
        }
        if (mem == SVO_MEM_DEVICE) {
            // straight into the caller's arrays
            rc = svo_orb_cv_launch(o, ptrs, nb, p.n_features, xy + 2 * nf * first, octave ? octave + nf * first : doct,
                                   response ? response + nf * first : dresp, dir ? dir + 2 * nf * first : ddir, desc + 8 * nf * first,
                                   dn_all + first, st);
            if (rc)
                return rc;
        } else {
            if ((rc = svo_orb_cv_launch(o, ptrs, nb, p.n_features, dxy, doct, dresp, ddir, ddesc, dn, st)))
                return rc;
            const size_t bytes = (size_t)B * nf * rec + (size_t)B * 4;
            if (hb.size() < bytes)
                hb.resize(bytes);
            SVO_HIP(hipMemcpyAsync(hb.data(), out.p, bytes, hipMemcpyDeviceToHost, st));
            SVO_HIP(hipStreamSynchronize(st));
            const unsigned char *b = hb.data();
            const unsigned char *b_oct = b + 8 * nf * B, *b_resp = b_oct + 4 * nf * B, *b_dir = b_resp + 4 * nf * B,
                                *b_desc = b_dir + 8 * nf * B, *b_n = b_desc + 32 * nf * B;
            for (int k = 0; k < nb; k++) {
                int hn;
                memcpy(&hn, b_n + 4 * k, 4);
                hn = hn < 0 ? 0 : (hn > p.n_features ? p.n_features : hn);
                n[first + k] = hn;
                const size_t i = (size_t)(first + k);
                memcpy(xy + 2 * nf * i, b + 8 * nf * k, (size_t)hn * 8);
                if (octave)
                    memcpy(octave + nf * i, b_oct + 4 * nf * k, (size_t)hn * 4);
                if (response)
                    memcpy(response + nf * i, b_resp + 4 * nf * k, (size_t)hn * 4);
                if (dir)
                    memcpy(dir + 2 * nf * i, b_dir + 8 * nf * k, (size_t)hn * 8);
                memcpy(desc + 8 * nf * i, b_desc + 32 * nf * k, (size_t)hn * 32);
            }
        }
    }
    if (mem == SVO_MEM_DEVICE) {
        SVO_HIP(hipMemcpyAsync(n, dn_all, (size_t)n_images * 4, hipMemcpyDeviceToHost, st));
        SVO_HIP(hipStreamSynchronize(st));
    }
    for (int i = 0; i < n_images; i++)
        n[i] = n[i] < 0 ? 0 : (n[i] > p.n_features ? p.n_features : n[i]);
    return SVO_OK;
}

}  // extern "C"
