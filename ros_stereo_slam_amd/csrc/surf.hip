// surf.hip -- OpenCV 3.2's xfeatures2d::SURF, detect and compute: the extractor of the older pipeline's
// visualOdometry::stereoTriangulate (src/bundleAdjust.cpp:236-317, SURF::create(500)) and of the SURF branch of
// visualSLAM::stereoTriangulate (include/trangulation.h:32-61, SURF::create(1200)).
//
// The algorithm is stated operation by operation in tests/surf_numpy.py (points U1 ... U10 as recalled from upstream, OURS-1 and
// OURS-2 where an order had to be fixed) and DESIGN.md section 10f; the kernels below are held to it bit for bit.  Every float
// operation is written as the restatement writes it (the library is built with -ffp-contract=off).
//
// Stages, all on the context's stream, blockIdx.y or .z = image of the batch, one host wait (for the counts):
//   1. grey image (BGR only) and the int32 integral image: the scans of integral_scan.hip.h, shared with brief.hip.
//   2. det / trace planes: one launch per octave fills every layer of it, a thread per sample, the ten box filters of the layer
//      resized once per workgroup into LDS.
//   3. maxima: one launch per octave over its middle layers; a thread per sample tests the threshold and the 26 neighbours,
//      interpolates (Cramer's rule in float), applies the two drops of the orientation stage that depend on position and size
//      alone, and appends through a wave ballot -- one atomic per wave.
//   4. order: every candidate counts the candidates that sort before it (the total order U8 + OURS-1) and writes its fields to
//      that place of the output: the append order of stage 3 can never show.
//   5. orientation: one wavefront per key point; the samples are gathered in order by ballots, lane k adds up windows k and
//      k + 64 in sample order (upstream's serial sums), lane 0 picks the first best window.
//   6. descriptor: one workgroup per key point.  The rotated window is never stored: thread t walks window rows t, t + 128, ...
//      with upstream's serial position updates and folds each row into 21 column sums (INTER_AREA's first pass) in LDS; after
//      every 128 rows the 441 patch cells take their rows in ascending order (its second pass).
#include <cmath>
#include <cstring>

#include "svo_internal.h"
#include "fast_atan2.hip.h"
#include "scan_ops.hip.h"

namespace {

#include "feature_batch.hip.h"
#include "integral_scan.hip.h"

constexpr int SURF_MAXBATCH = IMAGE_MAXBATCH, SURF_MAXOCT = 8, SURF_MAXCAND = 65536;
constexpr int SURF_ORI_RADIUS = 6, SURF_PATCH = 20, SURF_P1 = SURF_PATCH + 1;
constexpr int SURF_DESC_THREADS = 128;

struct SurfGeom {
    int w, h, n_oct, nl;             // nl: layers per octave = n_octave_layers + 2
    long long ooff[SURF_MAXOCT];     // floats from the start of an image's planes to those of octave o
    long long img_stride;            // floats per image
};
struct SurfWeights {
    float ori[2 * SURF_ORI_RADIUS + 1];   // getGaussianKernel(13, 2.5, CV_32F)
    float desc[SURF_PATCH];               // getGaussianKernel(20, 3.3, CV_32F)
};
struct SurfOut {
    float *xy, *size, *angle, *resp;
    int *oct, *lap;
    int cap;
};

__device__ __forceinline__ int surf_round(float v) { return (int)rintf(v); }

// U4: one box of a Haar pattern resized from `old_size` to `new_size` cells -> corners and weight
__device__ __forceinline__ void surf_resize_box(const int *src, int old_size, int new_size, int *box, float *wgt)
{
    const float ratio = (float)new_size / old_size;
    const int dx1 = surf_round(ratio * src[0]), dy1 = surf_round(ratio * src[1]);
    const int dx2 = surf_round(ratio * src[2]), dy2 = surf_round(ratio * src[3]);
    box[0] = dx1;
    box[1] = dy1;
    box[2] = dx2;
    box[3] = dy2;
    *wgt = src[4] / ((float)(dx2 - dx1) * (dy2 - dy1));
}

// the int box sum of U5 at origin p (pitch ints per row); unsigned: the intermediate sums may wrap, the result does not
__device__ __forceinline__ int surf_box(const int *__restrict__ p, int pitch, const int *box)
{
    const unsigned a = (unsigned)p[(size_t)box[1] * pitch + box[0]], d = (unsigned)p[(size_t)box[3] * pitch + box[2]];
    const unsigned b = (unsigned)p[(size_t)box[3] * pitch + box[0]], c = (unsigned)p[(size_t)box[1] * pitch + box[2]];
    return (int)(a + d - b - c);
}

// ---- 1. grey image ----
__global__ __launch_bounds__(256) void surf_grey_kernel(ImageBatch im, int n_px, uint8_t *__restrict__ grey_all, long long stride)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_px)
        return;
    const uint8_t *__restrict__ p = im.img[blockIdx.y] + 3 * (size_t)i;
    grey_all[blockIdx.y * stride + i] = (uint8_t)svo_bgr2gray(p[0], p[1], p[2]);
}

// ---- 2. det and trace of every layer of octave o (U3, U4, U5) ----
__global__ __launch_bounds__(256) void surf_layers_kernel(const int *__restrict__ sum_all, long long sum_stride, SurfGeom g, int o,
                                                          float *__restrict__ det_all, float *__restrict__ trace_all)
{
    const int pat[10][5] = {{0, 2, 3, 7, 1}, {3, 2, 6, 7, -2}, {6, 2, 9, 7, 1},                       // Dx
                            {2, 0, 7, 3, 1}, {2, 3, 7, 6, -2}, {2, 6, 7, 9, 1},                       // Dy
                            {1, 1, 4, 4, 1}, {5, 1, 8, 4, -1}, {1, 5, 4, 8, -1}, {5, 5, 8, 8, 1}};    // Dxy
    __shared__ int box[10][4];
    __shared__ float wgt[10];
    const int l = blockIdx.z % g.nl, b = blockIdx.z / g.nl;
    const int step = 1 << o, size = (9 + 6 * l) << o;
    if (size > g.w || size > g.h)
        return;   // the layer stays zero
    if (threadIdx.x < 10)
        surf_resize_box(pat[threadIdx.x], 9, size, box[threadIdx.x], &wgt[threadIdx.x]);
    __syncthreads();
    const int ni = 1 + (g.h - size) / step, nj = 1 + (g.w - size) / step, margin = (size / 2) / step;
    const int j = blockIdx.x * 64 + (threadIdx.x & 63), i = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (i >= ni || j >= nj)
        return;
    const int pitch = g.w + 1, lw = g.w >> o, lh = g.h >> o;
    const int *__restrict__ p = sum_all + b * sum_stride + (size_t)(i * step) * pitch + j * step;
    double d[3] = {0, 0, 0};
#pragma unroll
    for (int k = 0; k < 10; k++)
        d[k < 3 ? 0 : k < 6 ? 1 : 2] += (double)((float)surf_box(p, pitch, box[k]) * wgt[k]);
    const float dx = (float)d[0], dy = (float)d[1], dxy = (float)d[2];
    const size_t at = (size_t)b * g.img_stride + g.ooff[o] + (size_t)l * lw * lh + (size_t)(i + margin) * lw + (j + margin);
    det_all[at] = dx * dy - 0.81f * dxy * dxy;
    trace_all[at] = dx + dy;
}

// ---- 3. maxima (U6, U7, the drops of U9) ----
// U7: Matx33f::solve(b, DECOMP_LU) as recalled: Cramer's rule in float; a zero determinant gives x = 0
__device__ __forceinline__ void surf_solve3(const float a[3][3], const float b[3], float x[3])
{
    const float det = a[0][0] * (a[1][1] * a[2][2] - a[2][1] * a[1][2]) - a[0][1] * (a[1][0] * a[2][2] - a[2][0] * a[1][2]) +
                      a[0][2] * (a[1][0] * a[2][1] - a[2][0] * a[1][1]);
    if (det == 0) {
        x[0] = x[1] = x[2] = 0;
        return;
    }
    const float d = 1.f / det;
    x[0] = d * (b[0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (b[1] * a[2][2] - a[1][2] * b[2]) +
                a[0][2] * (b[1] * a[2][1] - a[1][1] * b[2]));
    x[1] = d * (a[0][0] * (b[1] * a[2][2] - a[1][2] * b[2]) - b[0] * (a[1][0] * a[2][2] - a[1][2] * a[2][0]) +
                a[0][2] * (a[1][0] * b[2] - b[1] * a[2][0]));
    x[2] = d * (a[0][0] * (a[1][1] * b[2] - b[1] * a[2][1]) - a[0][1] * (a[1][0] * b[2] - b[1] * a[2][0]) +
                b[0] * (a[1][0] * a[2][1] - a[1][1] * a[2][0]));
}

// U9: s, grad_wav_size and whether the wavelet fits the integral image at all.  OURS-3 (key points from elsewhere only): a
// position that is not finite or beyond +-65536, or a size whose window (int)(21 s) is not in 21 ... 65536, does not fit
__device__ __forceinline__ bool surf_scale(float x, float y, float size, int w, int h, float *s, int *gws)
{
    *s = size * 1.2f / 9.0f;
    *gws = 0;
    if (!(fabsf(x) <= 65536.f && fabsf(y) <= 65536.f && (SURF_PATCH + 1) * *s >= 21.f && (SURF_PATCH + 1) * *s <= 65536.f))
        return false;
    *gws = 2 * surf_round(2 * *s);
    return !(h + 1 < *gws || w + 1 < *gws);
}

// U9: sample (ai, aj) of the orientation stage -> the origin of its wavelets and whether it lies inside
__device__ __forceinline__ bool surf_ori_pos(float x, float y, float s, int gws, int ai, int aj, int w, int h, int *px, int *py)
{
    const float off = (float)(gws - 1) / 2;
    *px = surf_round(x + ai * s - off);
    *py = surf_round(y + aj * s - off);
    return !(*py < 0 || *py >= h + 1 - gws || *px < 0 || *px >= w + 1 - gws);
}

// does the orientation stage keep the key point (it depends on position and size alone)
__device__ bool surf_fits(float x, float y, float size, int w, int h, int upright)
{
    float s;
    int gws, px, py;
    if (!surf_scale(x, y, size, w, h, &s, &gws))
        return false;
    if (upright)
        return true;
    for (int i = -SURF_ORI_RADIUS; i <= SURF_ORI_RADIUS; i++)
        for (int j = -SURF_ORI_RADIUS; j <= SURF_ORI_RADIUS; j++)
            if (i * i + j * j <= SURF_ORI_RADIUS * SURF_ORI_RADIUS && surf_ori_pos(x, y, s, gws, i, j, w, h, &px, &py))
                return true;
    return false;
}

__global__ __launch_bounds__(256) void surf_maxima_kernel(const float *__restrict__ det_all, const float *__restrict__ trace_all,
                                                          SurfGeom g, int o, float thr, int upright, float4 *__restrict__ ka_all,
                                                          int4 *__restrict__ kb_all, int *__restrict__ lap_all,
                                                          int *__restrict__ count_all)
{
    const int nmid = g.nl - 2, l = 1 + blockIdx.z % nmid, b = blockIdx.z / nmid;
    const int step = 1 << o, size = (9 + 6 * l) << o, lw = g.w >> o, lh = g.h >> o;
    const int margin = ((((9 + 6 * (l + 1)) << o) / 2) / step) + 1;
    const int j = blockIdx.x * 64 + (threadIdx.x & 63), i = blockIdx.y * 4 + (threadIdx.x >> 6);
    bool found = false;
    float kx = 0, ky = 0, ksize = 0, val0 = 0;
    int lap = 0;
    if (i >= margin && i < lh - margin && j >= margin && j < lw - margin) {
        const size_t plane = (size_t)lw * lh;
        const float *__restrict__ c = det_all + (size_t)b * g.img_stride + g.ooff[o] + (size_t)l * plane + (size_t)i * lw + j;
        val0 = *c;
        if (val0 > thr) {
            float N9[3][9];
            bool is_max = true;
#pragma unroll
            for (int dl = 0; dl < 3; dl++)
#pragma unroll
                for (int k = 0; k < 9; k++) {
                    const float v = c[(ptrdiff_t)(dl - 1) * (ptrdiff_t)plane + (ptrdiff_t)(k / 3 - 1) * lw + (k % 3 - 1)];
                    N9[dl][k] = v;
                    if (!(dl == 1 && k == 4))
                        is_max = is_max && val0 > v;
                }
            if (is_max) {
                const float bb[3] = {-(N9[1][5] - N9[1][3]) / 2, -(N9[1][7] - N9[1][1]) / 2, -(N9[2][4] - N9[0][4]) / 2};
                const float axy = (N9[1][8] - N9[1][6] - N9[1][2] + N9[1][0]) / 4;
                const float axs = (N9[2][5] - N9[2][3] - N9[0][5] + N9[0][3]) / 4;
                const float ays = (N9[2][7] - N9[2][1] - N9[0][7] + N9[0][1]) / 4;
                const float A[3][3] = {{N9[1][3] - 2 * N9[1][4] + N9[1][5], axy, axs},
                                       {axy, N9[1][1] - 2 * N9[1][4] + N9[1][7], ays},
                                       {axs, ays, N9[0][4] - 2 * N9[1][4] + N9[2][4]}};
                float x[3];
                surf_solve3(A, bb, x);
                const bool ok = (x[0] != 0 || x[1] != 0 || x[2] != 0) && fabsf(x[0]) <= 1 && fabsf(x[1]) <= 1 && fabsf(x[2]) <= 1;
                if (ok) {
                    const float half = (size - 1) * 0.5f;
                    const int sum_i = step * (i - (size / 2) / step), sum_j = step * (j - (size / 2) / step);
                    const int ds = size - ((9 + 6 * (l - 1)) << o);
                    kx = (sum_j + half) + x[0] * step;
                    ky = (sum_i + half) + x[1] * step;
                    ksize = (float)surf_round(size + x[2] * ds);
                    found = surf_fits(kx, ky, ksize, g.w, g.h, upright);
                    const float t = trace_all[(size_t)b * g.img_stride + g.ooff[o] + (size_t)l * plane + (size_t)i * lw + j];
                    lap = (t > 0) - (t < 0);
                }
            }
        }
    }
    const unsigned long long m = __ballot(found);
    if (m == 0)
        return;
    const int lane = threadIdx.x & 63;
    int base = 0;
    if (lane == __ffsll((long long)m) - 1)
        base = atomicAdd(count_all + b, __popcll(m));
    base = __shfl(base, __ffsll((long long)m) - 1);
    if (found) {
        const int at = base + svo::lanes_below(m);
        if (at < SURF_MAXCAND) {
            const size_t q = (size_t)b * SURF_MAXCAND + at;
            ka_all[q] = make_float4(val0, ksize, ky, kx);
            kb_all[q] = make_int4(o, l, i, j);
            lap_all[q] = lap;
        }
    }
}

// ---- 4. order (U8, OURS-1) ----
// does a sort before b; ka = (response, size, y, x), kb = (octave, layer, row, column)
__device__ __forceinline__ bool surf_before(const float4 a, const int4 ai, const float4 b, const int4 bi)
{
    if (a.x != b.x)
        return a.x > b.x;
    if (a.y != b.y)
        return a.y > b.y;
    if (ai.x != bi.x)
        return ai.x > bi.x;
    if (a.z != b.z)
        return a.z > b.z;
    if (a.w != b.w)
        return a.w < b.w;
    if (ai.y != bi.y)
        return ai.y < bi.y;
    if (ai.z != bi.z)
        return ai.z < bi.z;
    return ai.w < bi.w;
}

__global__ __launch_bounds__(256) void surf_rank_kernel(const float4 *__restrict__ ka_all, const int4 *__restrict__ kb_all,
                                                        const int *__restrict__ lap_all, const int *__restrict__ count_all, SurfOut out)
{
    __shared__ float4 ta[256];
    __shared__ int4 tb[256];
    const int b = blockIdx.y, n = min(count_all[b], SURF_MAXCAND);
    if ((int)(blockIdx.x * 256) >= n)
        return;
    const float4 *__restrict__ ka = ka_all + (size_t)b * SURF_MAXCAND;
    const int4 *__restrict__ kb = kb_all + (size_t)b * SURF_MAXCAND;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool live = i < n;
    const float4 a = live ? ka[i] : make_float4(0, 0, 0, 0);
    const int4 ai = live ? kb[i] : make_int4(0, 0, 0, 0);
    int rank = 0;
    for (int j0 = 0; j0 < n; j0 += 256) {
        if (j0 + (int)threadIdx.x < n) {
            ta[threadIdx.x] = ka[j0 + threadIdx.x];
            tb[threadIdx.x] = kb[j0 + threadIdx.x];
        }
        __syncthreads();
        const int m = min(256, n - j0);
        for (int j = 0; j < m; j++)
            rank += surf_before(ta[j], tb[j], a, ai) ? 1 : 0;
        __syncthreads();
    }
    if (!live || rank >= out.cap)
        return;
    const size_t q = (size_t)b * out.cap + rank;
    out.xy[2 * q] = a.w;
    out.xy[2 * q + 1] = a.z;
    out.size[q] = a.y;
    out.resp[q] = a.x;
    out.oct[q] = ai.x;
    out.lap[q] = lap_all[(size_t)b * SURF_MAXCAND + i];
}

// ---- 5. orientation (U9): a wavefront per key point ----
// count: the images' live counts (the detector's) or null (n_fixed key points); kept (optional): 1 / 0 per key point
__global__ __launch_bounds__(256) void surf_orientation_kernel(const int *__restrict__ sum_all, long long sum_stride, int w, int h,
                                                               const float *__restrict__ xy_all, const float *__restrict__ size_all,
                                                               const int *__restrict__ count_all, int n_fixed, int cap, int upright,
                                                               SurfWeights wt, float *__restrict__ angle_all,
                                                               uint8_t *__restrict__ kept_all)
{
    constexpr int NS = 113, NW = 72;
    __shared__ float X[4][NS], Y[4][NS], SX[4][NW], SY[4][NW];
    __shared__ int A[4][NS];
    const int gx[2][5] = {{0, 0, 2, 4, -1}, {2, 0, 4, 4, 1}}, gy[2][5] = {{0, 0, 4, 2, 1}, {0, 2, 4, 4, -1}};
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.y;
    const int n = count_all ? min(count_all[b], cap) : n_fixed;
    const int k = blockIdx.x * 4 + wave;
    const bool live = k < n;
    const size_t q = (size_t)b * cap + (live ? k : 0);
    const float x = xy_all[2 * q], y = xy_all[2 * q + 1], size = size_all[q];
    float s;
    int gws;
    const bool fit = surf_scale(x, y, size, w, h, &s, &gws) && live;
    int nangle = 0;
    if (fit && !upright) {
        int bxs[4][4];
        float bws[4];
#pragma unroll
        for (int t = 0; t < 2; t++) {
            surf_resize_box(gx[t], 4, gws, bxs[t], &bws[t]);
            surf_resize_box(gy[t], 4, gws, bxs[2 + t], &bws[2 + t]);
        }
        const int pitch = w + 1;
        const int *__restrict__ sum = sum_all + b * sum_stride;
        for (int r = 0; r < 3; r++) {
            const int t = r * 64 + lane, ai = t / 13 - SURF_ORI_RADIUS, aj = t % 13 - SURF_ORI_RADIUS;
            int px = 0, py = 0;
            const bool ok = t < 169 && ai * ai + aj * aj <= SURF_ORI_RADIUS * SURF_ORI_RADIUS &&
                            surf_ori_pos(x, y, s, gws, ai, aj, w, h, &px, &py);
            const unsigned long long m = __ballot(ok);
            if (ok) {
                const int *__restrict__ p = sum + (size_t)py * pitch + px;
                double dx = 0, dy = 0;
#pragma unroll
                for (int u = 0; u < 2; u++) {
                    dx += (double)((float)surf_box(p, pitch, bxs[u]) * bws[u]);
                    dy += (double)((float)surf_box(p, pitch, bxs[2 + u]) * bws[2 + u]);
                }
                const float wgt = wt.ori[ai + SURF_ORI_RADIUS] * wt.ori[aj + SURF_ORI_RADIUS];
                const float vx = (float)dx * wgt, vy = (float)dy * wgt;
                const int at = nangle + svo::lanes_below(m);
                X[wave][at] = vx;
                Y[wave][at] = vy;
                A[wave][at] = surf_round(fast_atan2_deg(vy, vx));
            }
            nangle += __popcll(m);
        }
    }
    __syncthreads();
    const bool keep = fit && (upright || nangle > 0);
    if (keep && !upright)
        for (int wdw = lane; wdw < NW; wdw += 64) {
            const int i = 5 * wdw;
            float sumx = 0, sumy = 0;
            for (int j = 0; j < nangle; j++) {
                const int d = abs(A[wave][j] - i);
                if (d < 30 || d > 330) {
                    sumx += X[wave][j];
                    sumy += Y[wave][j];
                }
            }
            SX[wave][wdw] = sumx;
            SY[wave][wdw] = sumy;
        }
    __syncthreads();
    if (!live || lane != 0)
        return;
    float angle = -1.f;
    if (keep && upright) {
        angle = 270.f;
    } else if (keep) {
        float bestx = 0, besty = 0, best = 0;
        for (int wdw = 0; wdw < NW; wdw++) {
            const float sx = SX[wave][wdw], sy = SY[wave][wdw], mod = sx * sx + sy * sy;
            if (mod > best) {
                best = mod;
                bestx = sx;
                besty = sy;
            }
        }
        angle = fast_atan2_deg(-besty, bestx);
    }
    angle_all[q] = angle;
    if (kept_all)
        kept_all[q] = keep ? 1 : 0;
}

// ---- 6. descriptor (U10, OURS-2): a workgroup per key point ----
__device__ __forceinline__ int surf_win_pixel(const uint8_t *__restrict__ grey, int w, int h, double px, double py)
{
    const int ix = (int)floor(px), iy = (int)floor(py);
    if ((unsigned)ix < (unsigned)(w - 1) && (unsigned)iy < (unsigned)(h - 1)) {
        const float a = (float)(px - ix), b = (float)(py - iy);
        const uint8_t *__restrict__ p = grey + (size_t)iy * w + ix;
        return surf_round(p[0] * (1.f - a) * (1.f - b) + p[1] * a * (1.f - b) + p[w] * (1.f - a) * b + p[w + 1] * a * b);
    }
    const int x = min(max((int)rint(px), 0), w - 1), y = min(max((int)rint(py), 0), h - 1);
    return grey[(size_t)y * w + x];
}

__global__ __launch_bounds__(SURF_DESC_THREADS) void surf_describe_kernel(const uint8_t *__restrict__ grey_all, long long grey_stride, int w,
                                                                          int h, const float *__restrict__ xy_all,
                                                                          const float *__restrict__ size_all,
                                                                          const float *__restrict__ angle_all,
                                                                          const uint8_t *__restrict__ kept_all,
                                                                          const int *__restrict__ count_all, int n_fixed, int cap,
                                                                          int upright, SurfWeights wt, float *__restrict__ desc_all)
{
    constexpr int T = SURF_DESC_THREADS, NP = SURF_P1 * SURF_P1;
    __shared__ float buf[T][SURF_P1];
    __shared__ float acc[NP];
    __shared__ int patch[NP];
    __shared__ int t_sx1[SURF_P1], t_sx2[SURF_P1];
    __shared__ float t_al[SURF_P1], t_am[SURF_P1], t_ar[SURF_P1];   // a fraction of 0 = no such entry
    __shared__ float DX[SURF_PATCH * SURF_PATCH], DY[SURF_PATCH * SURF_PATCH], vec[64];
    __shared__ float s_scale;
    const int b = blockIdx.y, k = blockIdx.x, tid = threadIdx.x;
    const int n = count_all ? min(count_all[b], cap) : n_fixed;
    if (k >= n)
        return;
    const size_t q = (size_t)b * cap + k;
    float *__restrict__ desc = desc_all + 64 * q;
    if (kept_all && !kept_all[q]) {
        if (tid < 64)
            desc[tid] = 0;
        return;
    }
    const uint8_t *__restrict__ grey = grey_all + b * grey_stride;
    const float x = xy_all[2 * q], y = xy_all[2 * q + 1], s = size_all[q] * 1.2f / 9.0f;
    const int win = (int)((SURF_PATCH + 1) * s);
    // OURS-2: the area table of win -> 21, the same for columns and rows
    const double scale = 1.0 / (21.0 / win);
    const int kfast = fabs(scale - rint(scale)) < 2.220446049250313e-16 ? (int)rint(scale) : 0;
    if (tid < SURF_P1) {
        if (kfast) {
            t_sx1[tid] = tid * kfast;
            t_sx2[tid] = tid * kfast + kfast;
            t_al[tid] = 0;
            t_am[tid] = 1;
            t_ar[tid] = 0;
        } else {
            const double fsx1 = tid * scale, fsx2 = fsx1 + scale, cell = fmin(scale, win - fsx1);
            int sx1 = (int)ceil(fsx1), sx2 = (int)floor(fsx2);
            sx2 = min(sx2, win - 1);
            sx1 = min(sx1, sx2);
            t_sx1[tid] = sx1;
            t_sx2[tid] = sx2;
            t_al[tid] = sx1 - fsx1 > 1e-3 ? (float)((sx1 - fsx1) / cell) : 0.f;
            t_am[tid] = (float)(1.0 / cell);
            t_ar[tid] = fsx2 - sx2 > 1e-3 ? (float)(fmin(fmin(fsx2 - sx2, 1.), cell) / cell) : 0.f;
        }
    }
    for (int p = tid; p < NP; p += T)
        acc[p] = 0;
    // the window's geometry
    const float off = -(float)(win - 1) / 2;
    float sin_dir = 0, cos_dir = 0, rx = 0, ry = 0;
    int ux = 0, uy = 0;
    if (upright) {
        ux = surf_round(x + off);
        uy = surf_round(y - off);
    } else {
        const float rad = angle_all[q] * (float)(3.14159265358979323846 / 180);
        sin_dir = -(float)svo_sin((double)rad);
        cos_dir = (float)svo_cos((double)rad);
        rx = x + off * cos_dir + off * sin_dir;
        ry = y - off * sin_dir + off * cos_dir;
    }
    int cur_i = 0;
    __syncthreads();
    for (int r0 = 0; r0 < win; r0 += T) {
        const int i = r0 + tid;
        if (i < win) {
            for (; cur_i < i; cur_i++) {   // one float addition per row, as upstream's loop
                rx += sin_dir;
                ry += cos_dir;
            }
            double px = rx, py = ry;
            int cur_j = -1;
            float cur_v = 0;
            auto get = [&](int j) {
                while (cur_j < j) {
                    if (cur_j >= 0) {   // one double addition per column
                        px += (double)cos_dir;
                        py -= (double)sin_dir;
                    }
                    cur_j++;
                    if (upright)
                        cur_v = (float)grey[(size_t)min(max(uy - cur_j, 0), h - 1) * w + min(max(ux + i, 0), w - 1)];
                    else
                        cur_v = (float)surf_win_pixel(grey, w, h, px, py);
                }
                return cur_v;
            };
            for (int dx = 0; dx < SURF_P1; dx++) {
                const int sx1 = t_sx1[dx], sx2 = t_sx2[dx];
                const float al = t_al[dx], am = t_am[dx], ar = t_ar[dx];
                float v = 0;
                if (al != 0)
                    v = v + get(sx1 - 1) * al;
                for (int sx = sx1; sx < sx2; sx++)
                    v = v + get(sx) * am;
                if (ar != 0)
                    v = v + get(sx2) * ar;
                buf[tid][dx] = v;
            }
        }
        __syncthreads();
        const int r1 = min(r0 + T, win);
        for (int p = tid; p < NP; p += T) {
            const int dy = p / SURF_P1, dx = p % SURF_P1, sy1 = t_sx1[dy], sy2 = t_sx2[dy];
            float a = acc[p];
            if (t_al[dy] != 0 && sy1 - 1 >= r0 && sy1 - 1 < r1)
                a = a + t_al[dy] * buf[sy1 - 1 - r0][dx];
            for (int sy = max(sy1, r0); sy < min(sy2, r1); sy++)
                a = a + t_am[dy] * buf[sy - r0][dx];
            if (t_ar[dy] != 0 && sy2 >= r0 && sy2 < r1)
                a = a + t_ar[dy] * buf[sy2 - r0][dx];
            acc[p] = a;
        }
        __syncthreads();
    }
    for (int p = tid; p < NP; p += T) {
        int v;
        if (kfast == 2)
            v = ((int)acc[p] + 2) >> 2;
        else if (kfast)
            v = surf_round((float)(int)acc[p] * (1.f / (float)(kfast * kfast)));
        else
            v = surf_round(acc[p]);
        patch[p] = min(max(v, 0), 255);
    }
    __syncthreads();
    for (int p = tid; p < SURF_PATCH * SURF_PATCH; p += T) {
        const int i = p / SURF_PATCH, j = p % SURF_PATCH;
        const float dw = wt.desc[i] * wt.desc[j];
        const int p00 = patch[i * SURF_P1 + j], p01 = patch[i * SURF_P1 + j + 1], p10 = patch[(i + 1) * SURF_P1 + j],
                  p11 = patch[(i + 1) * SURF_P1 + j + 1];
        DX[p] = (float)(p01 - p00 + p11 - p10) * dw;
        DY[p] = (float)(p10 - p00 + p11 - p01) * dw;
    }
    __syncthreads();
    if (tid < 64) {
        const int cell = tid >> 2, comp = tid & 3, ci = cell >> 2, cj = cell & 3;
        float v = 0;
        for (int yy = ci * 5; yy < ci * 5 + 5; yy++)
            for (int xx = cj * 5; xx < cj * 5 + 5; xx++) {
                const float t = (comp & 1) ? DY[yy * SURF_PATCH + xx] : DX[yy * SURF_PATCH + xx];
                v += comp < 2 ? t : fabsf(t);
            }
        vec[tid] = v;
    }
    __syncthreads();
    if (tid == 0) {
        double sq = 0;
        for (int t = 0; t < 64; t++)
            sq += (double)(vec[t] * vec[t]);
        s_scale = (float)(1. / (sqrt(sq) + (double)1.1920928955078125e-07f));
    }
    __syncthreads();
    if (tid < 64)
        desc[tid] = vec[tid] * s_scale;
}

// ---- host side ----
// U9: getGaussianKernel(n, sigma, CV_32F), n > 7
void surf_gaussian(int n, double sigma, float *c)
{
    const double scale2x = -0.5 / (sigma * sigma);
    double sum = 0;
    for (int i = 0; i < n; i++) {
        const double x = i - (n - 1) * 0.5;
        c[i] = (float)svo_exp(scale2x * x * x);
        sum += c[i];
    }
    sum = 1. / sum;
    for (int i = 0; i < n; i++)
        c[i] = (float)(c[i] * sum);
}

SurfWeights surf_weights()
{
    SurfWeights wt;
    surf_gaussian(2 * SURF_ORI_RADIUS + 1, 2.5, wt.ori);
    surf_gaussian(SURF_PATCH, 3.3, wt.desc);
    return wt;
}

int surf_check(const svo_surf_params *prm, svo_surf_params &p, int w, int h, int c)
{
    svo_surf_default_params(&p);
    if (prm)
        p = *prm;
    SVO_CHECK_ARG(c == 1 || c == 3);
    SVO_CHECK_ARG(w >= 1 && h >= 1 && w <= 16384 && h <= 16384);
    SVO_CHECK_ARG(p.n_octaves >= 1 && p.n_octaves <= SURF_MAXOCT && p.n_octave_layers >= 1 && p.n_octave_layers <= 8);
    SVO_CHECK_ARG(std::isfinite(p.hessian_threshold) && p.hessian_threshold >= 0);
    if (p.extended != 0) {
        svo_set_error("svo_surf: extended (128-float) descriptors are not provided");
        return SVO_ERR_ARG;
    }
    if (!integral_fits_int32(w, h)) {
        svo_set_error("svo_surf: the int32 integral image of %d x %d pixels could overflow (255 w h > 2^31 - 1)", w, h);
        return SVO_ERR_ARG;
    }
    return SVO_OK;
}

SurfGeom surf_geom(int w, int h, const svo_surf_params &p)
{
    SurfGeom g;
    memset(&g, 0, sizeof(g));
    g.w = w;
    g.h = h;
    g.n_oct = p.n_octaves;
    g.nl = p.n_octave_layers + 2;
    long long off = 0;
    for (int o = 0; o < g.n_oct; o++) {
        g.ooff[o] = off;
        off += (long long)g.nl * (w >> o) * (h >> o);
    }
    g.img_stride = (off + 63) & ~63ll;
    return g;
}

struct SurfPlan {
    SurfGeom g;
    long long sum_stride, grey_stride;
    const int *sum;
    const uint8_t *grey;
    float *det, *trace;
};

// grey images, integral images and (planes) the det / trace planes of nb device images
int surf_prepare(svo_ctx *ctx, const uint8_t *const *d_images, int nb, int w, int h, int c, const svo_surf_params &p, bool planes,
                 SurfPlan &pl)
{
    hipStream_t st = ctx->stream;
    pl.g = surf_geom(w, h, p);
    pl.sum_stride = integral_img_stride(w, h);
    pl.grey_stride = ((long long)w * h + 255) & ~255ll;
    int rc;
    // the scans are queued before the grey kernel and the gather: all three only read the images, and the grey planes lie in the
    // buffer integral_images sizes
    if ((rc = integral_images(ctx, d_images, nb, w, h, c, c == 3 ? (size_t)pl.grey_stride * nb : 0)))
        return rc;
    pl.sum = ctx->feat_sum.as<int>();
    if (c == 3) {
        uint8_t *grey = ctx->feat_sum.as<uint8_t>() + (size_t)pl.sum_stride * nb * 4;
        hipLaunchKernelGGL(surf_grey_kernel, dim3((w * h + 255) / 256, nb), dim3(256), 0, st, make_image_batch(d_images, nb), w * h, grey,
                           pl.grey_stride);
        pl.grey = grey;
    } else {
        // grey images of a batch need not be evenly spaced: the descriptor kernel takes image 0's address and a stride, so a
        // batch of separate grey images is gathered as well
        bool even = true;
        for (int k = 1; k < nb; k++)
            even = even && d_images[k] - d_images[0] == (ptrdiff_t)k * (d_images[1] - d_images[0]);
        if (nb == 1 || even) {
            pl.grey = d_images[0];
            pl.grey_stride = nb > 1 ? (long long)(d_images[1] - d_images[0]) : 0;
        } else {
            // device images only (staged host images are evenly spaced), so ctx->feat_img holds nothing of this call yet
            if ((rc = ctx->feat_img.ensure((size_t)pl.grey_stride * nb + 256)))
                return rc;
            for (int k = 0; k < nb; k++)
                SVO_HIP(hipMemcpyAsync(ctx->feat_img.as<uint8_t>() + (size_t)k * pl.grey_stride, d_images[k], (size_t)w * h,
                                       hipMemcpyDeviceToDevice, st));
            pl.grey = ctx->feat_img.as<uint8_t>();
        }
    }
    SVO_HIP(hipGetLastError());
    pl.det = pl.trace = nullptr;
    if (!planes)
        return SVO_OK;
    const size_t pf = (size_t)pl.g.img_stride * nb;
    if ((rc = ctx->surf_planes.ensure(2 * pf * 4 + 256)))
        return rc;
    pl.det = ctx->surf_planes.as<float>();
    pl.trace = pl.det + pf;
    SVO_HIP(hipMemsetAsync(pl.det, 0, 2 * pf * 4, st));
    for (int o = 0; o < pl.g.n_oct; o++) {
        const int lw = w >> o, lh = h >> o;
        if (lw < 1 || lh < 1)
            break;
        hipLaunchKernelGGL(surf_layers_kernel, dim3((lw + 63) / 64, (lh + 3) / 4, pl.g.nl * nb), dim3(256), 0, st, pl.sum, pl.sum_stride,
                           pl.g, o, pl.det, pl.trace);
    }
    SVO_HIP(hipGetLastError());
    return SVO_OK;
}

}  // namespace

extern "C" {

void svo_surf_default_params(svo_surf_params *p)
{
    if (!p)
        return;
    p->hessian_threshold = 100;   // SURF::create()
    p->n_octaves = 4;
    p->n_octave_layers = 3;
    p->extended = 0;
    p->upright = 0;
}

int svo_surf_layers_layout(int w, int h, int n_octaves, int n_octave_layers, int *sizes, int *steps, int *lw, int *lh)
{
    SVO_CHECK_ARG(w >= 1 && h >= 1 && w <= 16384 && h <= 16384);
    SVO_CHECK_ARG(n_octaves >= 1 && n_octaves <= SURF_MAXOCT && n_octave_layers >= 1 && n_octave_layers <= 8);
    for (int o = 0, k = 0; o < n_octaves; o++)
        for (int l = 0; l < n_octave_layers + 2; l++, k++) {
            if (sizes)
                sizes[k] = (9 + 6 * l) << o;
            if (steps)
                steps[k] = 1 << o;
            if (lw)
                lw[k] = w >> o;
            if (lh)
                lh[k] = h >> o;
        }
    return SVO_OK;
}

int svo_surf_layers(svo_ctx *ctx, const uint8_t *image, int w, int h, int c, const svo_surf_params *prm, float *det, float *trace,
                    int mem)
{
    SVO_CHECK_ARG(ctx && image && det && trace && aligned4(det) && aligned4(trace));
    SVO_CHECK_ARG(mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE);
    svo_surf_params p;
    int rc;
    if ((rc = surf_check(prm, p, w, h, c)))
        return rc;
    SVO_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint8_t *d_img = nullptr;
    SurfPlan pl;
    if ((rc = stage_images(ctx, &image, 1, (size_t)w * h * c, mem, &d_img)) || (rc = surf_prepare(ctx, &d_img, 1, w, h, c, p, true, pl)))
        return rc;
    const SurfGeom &g = pl.g;
    const int last = g.n_oct - 1;
    const size_t nf = (size_t)g.ooff[last] + (size_t)g.nl * (w >> last) * (h >> last);
    const hipMemcpyKind kind = mem == SVO_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (nf) {
        SVO_HIP(hipMemcpyAsync(det, pl.det, nf * 4, kind, st));
        SVO_HIP(hipMemcpyAsync(trace, pl.trace, nf * 4, kind, st));
    }
    if (mem == SVO_MEM_HOST)
        SVO_HIP(hipStreamSynchronize(st));
    return SVO_OK;
}

int svo_surf_extract_batch(svo_ctx *ctx, const uint8_t *const *images, int n_images, int w, int h, int c, const svo_surf_params *prm,
                           int cap, float *xy, float *size, float *angle, float *response, int *octave, int *laplacian, float *desc,
                           int *n, int mem)
{
    SVO_CHECK_ARG(ctx && images && n && xy && size && angle && response && octave && laplacian);
    SVO_CHECK_ARG(n_images >= 1 && n_images <= SURF_MAXBATCH && cap >= 1);
    SVO_CHECK_ARG(mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE);
    SVO_CHECK_ARG(aligned4(xy) && aligned4(size) && aligned4(angle) && aligned4(response) && aligned4(octave) && aligned4(laplacian) &&
                  aligned4(desc) && aligned4(n));
    for (int k = 0; k < n_images; k++)
        SVO_CHECK_ARG(images[k] != nullptr);
    svo_surf_params p;
    int rc;
    if ((rc = surf_check(prm, p, w, h, c)))
        return rc;
    SVO_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const bool host = mem == SVO_MEM_HOST;
    const size_t e = (size_t)n_images * cap, nc = (size_t)n_images * SURF_MAXCAND;
    const uint8_t *ptrs[SURF_MAXBATCH];
    if ((rc = stage_images(ctx, images, n_images, (size_t)w * h * c, mem, ptrs)))
        return rc;
    if ((rc = ctx->surf_work.ensure(256 + nc * (16 + 16 + 4) + 3 * 256 + (host ? e * (7 + (desc ? 64 : 0)) * 4 + 8 * 256 : 0))))
        return rc;
    uint8_t *q = ctx->surf_work.as<uint8_t>();
    int *d_counts = bump<int>(q, SURF_MAXBATCH);
    float4 *ka = bump<float4>(q, nc);
    int4 *kb = bump<int4>(q, nc);
    int *lap = bump<int>(q, nc);
    SurfOut out{xy, size, angle, response, octave, laplacian, cap};
    float *d_desc = desc;
    if (host) {
        out.xy = bump<float>(q, 2 * e);
        out.size = bump<float>(q, e);
        out.angle = bump<float>(q, e);
        out.resp = bump<float>(q, e);
        out.oct = bump<int>(q, e);
        out.lap = bump<int>(q, e);
        d_desc = desc ? bump<float>(q, 64 * e) : nullptr;
    }
    SurfPlan pl;
    if ((rc = surf_prepare(ctx, ptrs, n_images, w, h, c, p, true, pl)))
        return rc;
    SVO_HIP(hipMemsetAsync(d_counts, 0, sizeof(int) * SURF_MAXBATCH, st));
    for (int o = 0; o < pl.g.n_oct; o++) {
        const int lw = w >> o, lh = h >> o;
        if (lw < 1 || lh < 1)
            break;
        hipLaunchKernelGGL(surf_maxima_kernel, dim3((lw + 63) / 64, (lh + 3) / 4, p.n_octave_layers * n_images), dim3(256), 0, st,
                           pl.det, pl.trace, pl.g, o, (float)p.hessian_threshold, p.upright ? 1 : 0, ka, kb, lap, d_counts);
    }
    hipLaunchKernelGGL(surf_rank_kernel, dim3(SURF_MAXCAND / 256, n_images), dim3(256), 0, st, ka, kb, lap, d_counts, out);
    const SurfWeights wt = surf_weights();
    hipLaunchKernelGGL(surf_orientation_kernel, dim3((cap + 3) / 4, n_images), dim3(256), 0, st, pl.sum, pl.sum_stride, w, h, out.xy,
                       out.size, d_counts, 0, cap, p.upright ? 1 : 0, wt, out.angle, (uint8_t *)nullptr);
    if (d_desc)
        hipLaunchKernelGGL(surf_describe_kernel, dim3(cap, n_images), dim3(SURF_DESC_THREADS), 0, st, pl.grey, pl.grey_stride, w, h, out.xy,
                           out.size, out.angle, (const uint8_t *)nullptr, d_counts, 0, cap, p.upright ? 1 : 0, wt, d_desc);
    SVO_HIP(hipGetLastError());
    // the one wait: the counts
    if ((rc = read_counts(ctx, d_counts, n_images, n)))
        return rc;
    for (int k = 0; k < n_images; k++) {
        if (n[k] > SURF_MAXCAND) {
            svo_set_error("svo_surf_extract_batch: image %d has %d key points (the work arrays hold %d)", k, n[k], SURF_MAXCAND);
            return SVO_ERR_CAPACITY;
        }
        if (n[k] > cap && rc == SVO_OK) {
            svo_set_error("svo_surf_extract_batch: image %d yields %d key points, cap is %d", k, n[k], cap);
            rc = SVO_ERR_CAPACITY;
        }
    }
    if (host) {
        const HostColumn cols[7] = {{xy, out.xy, 8},      {size, out.size, 4},     {angle, out.angle, 4}, {response, out.resp, 4},
                                    {octave, out.oct, 4}, {laplacian, out.lap, 4}, {desc, d_desc, 64 * sizeof(float)}};
        const int rc_copy = copy_rows_to_host(st, cols, 7, n_images, cap, n);
        if (rc_copy)
            return rc_copy;
    }
    return rc;
}

int svo_surf_describe(svo_ctx *ctx, const uint8_t *image, int w, int h, int c, const svo_surf_params *prm, const float *xy,
                      const float *size, int n, float *angle_out, float *desc, uint8_t *kept, int mem)
{
    SVO_CHECK_ARG(ctx && image && n >= 0 && (n == 0 || (xy && size && angle_out && desc && kept)));
    SVO_CHECK_ARG(mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE);
    SVO_CHECK_ARG(aligned4(xy) && aligned4(size) && aligned4(angle_out) && aligned4(desc));
    svo_surf_params p;
    int rc;
    if ((rc = surf_check(prm, p, w, h, c)))
        return rc;
    if (n == 0)
        return SVO_OK;
    SVO_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const bool host = mem == SVO_MEM_HOST;
    const size_t e = (size_t)n;
    const uint8_t *d_img = nullptr;
    const float *dxy = xy, *dsize = size;
    float *dang = angle_out, *ddesc = desc;
    uint8_t *dkept = kept;
    if ((rc = stage_images(ctx, &image, 1, (size_t)w * h * c, mem, &d_img)))
        return rc;
    if (host) {
        if ((rc = ctx->surf_work.ensure(e * (4 * 68 + 1) + 6 * 256)))
            return rc;
        uint8_t *q = ctx->surf_work.as<uint8_t>();
        float *a = bump<float>(q, 2 * e), *b = bump<float>(q, e);
        dang = bump<float>(q, e);
        ddesc = bump<float>(q, 64 * e);
        dkept = bump<uint8_t>(q, e);
        SVO_HIP(hipMemcpyAsync(a, xy, e * 8, hipMemcpyHostToDevice, st));
        SVO_HIP(hipMemcpyAsync(b, size, e * 4, hipMemcpyHostToDevice, st));
        dxy = a;
        dsize = b;
    }
    SurfPlan pl;
    if ((rc = surf_prepare(ctx, &d_img, 1, w, h, c, p, false, pl)))
        return rc;
    const SurfWeights wt = surf_weights();
    hipLaunchKernelGGL(surf_orientation_kernel, dim3((n + 3) / 4, 1), dim3(256), 0, st, pl.sum, pl.sum_stride, w, h, dxy, dsize,
                       (const int *)nullptr, n, n, p.upright ? 1 : 0, wt, dang, dkept);
    hipLaunchKernelGGL(surf_describe_kernel, dim3(n, 1), dim3(SURF_DESC_THREADS), 0, st, pl.grey, pl.grey_stride, w, h, dxy, dsize, dang,
                       dkept, (const int *)nullptr, n, n, p.upright ? 1 : 0, wt, ddesc);
    SVO_HIP(hipGetLastError());
    if (host) {
        SVO_HIP(hipMemcpyAsync(angle_out, dang, e * 4, hipMemcpyDeviceToHost, st));
        SVO_HIP(hipMemcpyAsync(desc, ddesc, e * 256, hipMemcpyDeviceToHost, st));
        SVO_HIP(hipMemcpyAsync(kept, dkept, e, hipMemcpyDeviceToHost, st));
        SVO_HIP(hipStreamSynchronize(st));
    }
    return SVO_OK;
}

}  // extern "C"
