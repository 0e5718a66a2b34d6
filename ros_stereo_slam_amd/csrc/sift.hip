// sift.hip -- detection and descriptors of OpenCV 3.2's xfeatures2d::SIFT, the extractor behind
// StereoProcess::monocularTriangulate (src/StereoCV.cpp:123-147: SIFT::create(10000) -> detect / compute -> BFMatcher).
//
// The algorithm is stated operation by operation in tests/sift_numpy.py (points S1 ... S20 as recalled from upstream,
// OURS-1 ... OURS-4 where upstream leaves the result open) and DESIGN.md section 10d; this file follows it to the bit:
// float32 image arithmetic with one rounding per operation (-ffp-contract=off), exp / cos / sin from include/svo_math.h,
// the angle polynomial of fast_atan2.hip.h, histogram sums as exact integer sums (OURS-3), output in key order (OURS-4).
//
// Stages, all on the context's stream, `blockIdx.z` or `.y` = image of the batch, no host wait before the counts come back:
//   1. scale space: grey + 2x bilinear upsample (one kernel), then per layer a row pass and a column pass; the column pass
//      that produces layer i also writes DoG layer i - 1.  Octave bases are decimations of layer nOctaveLayers.
//   2. extrema: one lane per DoG pixel; a lane that finds a 26-neighbour extremum runs the sub-pixel refinement itself and
//      marks the cell its refinement ENDS in (a byte map over layer x row x column).  What a key point carries depends on
//      that cell only, so several starts that end in one cell write the same byte: removeDuplicated without a sort.
//   3. an ordered compaction of the byte map (block sums, scan of the sums, emit; the block scans are scan_ops.hip.h's) lists
//      the cells in (octave, layer, row, column) order -- the output order of the recipe falls out of the scan.
//   4. orientation: one wavefront per cell; the 36-bin histogram in LDS, peaks by ballot, in bin order.
//   5. a second ordered compaction expands the peaks, a radix selection on the response bits finds retainBest's threshold,
//      a third compaction keeps responses at or above it and writes the public fields (halved for the doubled octave).
//   6. descriptors: one wavefront per key point, 6 x 6 x 10 integer histogram in LDS.
#include <cmath>
#include <cstring>
#include <vector>

#include "svo_internal.h"
#include "fast_atan2.hip.h"
#include "scan_ops.hip.h"
#include "wave_ops.hip.h"

namespace {

#include "feature_batch.hip.h"

constexpr int SIFT_MAXOCT = 16, SIFT_MAXBATCH = IMAGE_MAXBATCH, SIFT_BORDER = 5, SIFT_STEPS = 5, SIFT_ORI_BINS = 36, SIFT_MAXPEAK = 18;
constexpr int SIFT_KP_CAP = 1 << 16;    // refined cells per image
constexpr int SIFT_ORI_CAP = 1 << 17;   // oriented key points per image before retainBest
constexpr int SIFT_KSTRIDE = 256;       // floats per Gaussian kernel (ksize <= 255)
constexpr int SCAN_T = 256, SCAN_ITEMS = 16, SCAN_BLOCK = SCAN_T * SCAN_ITEMS;
constexpr double SIFT_LN2 = 0.6931471805599453, SIFT_Q = 1048576.0, SIFT_QINV = 1.0 / 1048576.0;

struct SiftGeom {
    int no, nl;
    int w[SIFT_MAXOCT], h[SIFT_MAXOCT];
    long long goff[SIFT_MAXOCT], doff[SIFT_MAXOCT];   // floats, inside an image's block: nl + 3 / nl + 2 planes per octave
    int coff[SIFT_MAXOCT + 1];                        // cells (nl planes per octave) before octave o
    long long g_img, d_img;                           // floats per image
    int cells_img;                                    // bytes per image of the cell map (a multiple of 16)
};

// the taps of one blur, a kernel argument: every lane reads tap t at the same time, so they come in through scalar loads
struct SiftTaps {
    float k[SIFT_KSTRIDE];
};

__device__ __forceinline__ int reflect101(int p, int n)
{
    if (n == 1)
        return 0;
    while ((unsigned)p >= (unsigned)n)
        p = p < 0 ? -p : 2 * (n - 1) - p;
    return p;
}

// ---- 1. scale space ----
__device__ __forceinline__ void linear_tab(int d, int n, int &s0, int &s1, float &a0, float &a1)
{
    float fx = (float)((d + 0.5) * 0.5 - 0.5);
    int sx = (int)floorf(fx);
    fx = fx - (float)sx;
    if (sx < 0) {
        sx = 0;
        fx = 0.f;
    }
    if (sx >= n - 1) {
        sx = n - 1;
        fx = 0.f;
    }
    s0 = sx;
    s1 = sx + 1 < n ? sx + 1 : n - 1;
    a0 = 1.f - fx;
    a1 = fx;
}

__global__ __launch_bounds__(256) void sift_init_kernel(ImageBatch im, int w, int h, int c, float *__restrict__ base_all,
                                                        long long img_stride)
{
    const int dx = blockIdx.x * 256 + threadIdx.x, dy = blockIdx.y;
    if (dx >= 2 * w)
        return;
    const uint8_t *__restrict__ img = im.img[blockIdx.z];
    int x0, x1, y0, y1;
    float a0, a1, b0, b1;
    linear_tab(dx, w, x0, x1, a0, a1);
    linear_tab(dy, h, y0, y1, b0, b1);
    auto grey = [&](int y, int x) -> float {
        const size_t i = (size_t)y * w + x;
        if (c == 1)
            return (float)img[i];
        return (float)svo_bgr2gray(img[3 * i], img[3 * i + 1], img[3 * i + 2]);
    };
    const float t0 = grey(y0, x0) * a0 + grey(y0, x1) * a1;
    const float t1 = grey(y1, x0) * a0 + grey(y1, x1) * a1;
    base_all[blockIdx.z * img_stride + (size_t)dy * (2 * w) + dx] = t0 * b0 + t1 * b1;
}

// row pass: taps in index order (OURS-2)
__global__ __launch_bounds__(256) void sift_blur_row_kernel(const float *__restrict__ src_all, long long src_stride,
                                                            float *__restrict__ dst_all, long long dst_stride, int w, int h,
                                                            SiftTaps taps, int ks)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= w)
        return;
    const float *k = taps.k;
    const float *__restrict__ row = src_all + blockIdx.z * src_stride + (size_t)y * w;
    const int r = ks >> 1;
    float acc;
    if (x - r >= 0 && x + r < w) {
        const float *p = row + (x - r);
        acc = k[0] * p[0];
        for (int t = 1; t < ks; t++)
            acc = acc + k[t] * p[t];
    } else {
        acc = k[0] * row[reflect101(x - r, w)];
        for (int t = 1; t < ks; t++)
            acc = acc + k[t] * row[reflect101(x - r + t, w)];
    }
    dst_all[blockIdx.z * dst_stride + (size_t)y * w + x] = acc;
}

// column pass; dog (optional) = this layer - prev layer
__global__ __launch_bounds__(256) void sift_blur_col_kernel(const float *__restrict__ src_all, long long src_stride,
                                                            float *__restrict__ dst_all, const float *__restrict__ prev_all,
                                                            long long g_stride, float *__restrict__ dog_all, long long d_stride,
                                                            int w, int h, SiftTaps taps, int ks)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= w)
        return;
    const float *k = taps.k;
    const float *__restrict__ src = src_all + blockIdx.z * src_stride + x;
    const int r = ks >> 1;
    float acc;
    if (y - r >= 0 && y + r < h) {
        const float *p = src + (size_t)(y - r) * w;
        acc = k[0] * p[0];
        for (int t = 1; t < ks; t++)
            acc = acc + k[t] * p[(size_t)t * w];
    } else {
        acc = k[0] * src[(size_t)reflect101(y - r, h) * w];
        for (int t = 1; t < ks; t++)
            acc = acc + k[t] * src[(size_t)reflect101(y - r + t, h) * w];
    }
    const size_t i = (size_t)y * w + x;
    dst_all[blockIdx.z * g_stride + i] = acc;
    if (dog_all)
        dog_all[blockIdx.z * d_stride + i] = acc - prev_all[blockIdx.z * g_stride + i];
}

__global__ __launch_bounds__(256) void sift_decimate_kernel(const float *__restrict__ src_all, float *__restrict__ dst_all,
                                                            long long g_stride, int sw, int dw, int dh)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= dw)
        return;
    dst_all[blockIdx.z * g_stride + (size_t)y * dw + x] = src_all[blockIdx.z * g_stride + (size_t)(2 * y) * sw + 2 * x];
}

// ---- 2. extrema and refinement ----
struct SiftDeriv {
    float v, d0, d1, d2, dxx, dyy, dss, dxy, dxs, dys;
};

__device__ __forceinline__ SiftDeriv sift_derivs(const float *__restrict__ D, int w, size_t plane, int l, int r, int c)
{
    const float img_scale = 1.f / 255.f, ds = img_scale * 0.5f, ss = img_scale, cs = img_scale * 0.25f;
    const float *img = D + (size_t)l * plane + (size_t)r * w + c, *prv = img - plane, *nxt = img + plane;
    SiftDeriv d;
    d.v = img[0];
    d.d0 = (img[1] - img[-1]) * ds;
    d.d1 = (img[w] - img[-w]) * ds;
    d.d2 = (nxt[0] - prv[0]) * ds;
    const float v2 = d.v * 2.f;
    d.dxx = (img[1] + img[-1] - v2) * ss;
    d.dyy = (img[w] + img[-w] - v2) * ss;
    d.dss = (nxt[0] + prv[0] - v2) * ss;
    d.dxy = (img[w + 1] - img[w - 1] - img[-w + 1] + img[-w - 1]) * cs;
    d.dxs = (nxt[1] - nxt[-1] - prv[1] + prv[-1]) * cs;
    d.dys = (nxt[w] - nxt[-w] - prv[w] + prv[-w]) * cs;
    return d;
}

// Matx33f::solve(DECOMP_LU) = Cramer's rule in float; xi / xr / xc are the negated solution
__device__ __forceinline__ void sift_solve(const SiftDeriv &d, float &xi, float &xr, float &xc)
{
    const float a00 = d.dxx, a01 = d.dxy, a02 = d.dxs, a10 = d.dxy, a11 = d.dyy, a12 = d.dys, a20 = d.dxs, a21 = d.dys, a22 = d.dss;
    const float b0 = d.d0, b1 = d.d1, b2 = d.d2;
    const float det = a00 * (a11 * a22 - a12 * a21) - a01 * (a10 * a22 - a12 * a20) + a02 * (a10 * a21 - a11 * a20);
    if (det == 0.f) {
        xi = xr = xc = -0.f;
        return;
    }
    const float dd = 1.f / det;
    const float x0 = dd * (b0 * (a11 * a22 - a12 * a21) - a01 * (b1 * a22 - a12 * b2) + a02 * (b1 * a21 - a11 * b2));
    const float x1 = dd * (a00 * (b1 * a22 - a12 * b2) - b0 * (a10 * a22 - a12 * a20) + a02 * (a10 * b2 - b1 * a20));
    const float x2 = dd * (a00 * (a11 * b2 - b1 * a21) - a01 * (a10 * b2 - b1 * a20) + b0 * (a10 * a21 - a11 * a20));
    xi = -x2;
    xr = -x1;
    xc = -x0;
}

__device__ __forceinline__ bool sift_accept(const SiftDeriv &d, float xi, float xr, float xc, int nl, float cthr, float ethr,
                                            float *contr_out)
{
    const float t = d.d0 * xc + d.d1 * xr + d.d2 * xi;
    const float contr = d.v * (1.f / 255.f) + t * 0.5f;
    if (contr_out)
        *contr_out = contr;
    if (fabsf(contr) * (float)nl < cthr)
        return false;
    const float tr = d.dxx + d.dyy, det = d.dxx * d.dyy - d.dxy * d.dxy;
    if (det <= 0.f || tr * tr * ethr >= (ethr + 1.f) * (ethr + 1.f) * det)
        return false;
    return true;
}

// grid (ceil((w - 10) / 256), h - 10, batch * nl)
__global__ __launch_bounds__(256) void sift_extrema_kernel(SiftGeom g, int o, const float *__restrict__ dog_all,
                                                           uint8_t *__restrict__ flags_all, float thr, float cthr, float ethr)
{
    const int w = g.w[o], h = g.h[o], nl = g.nl;
    const int c = blockIdx.x * 256 + threadIdx.x + SIFT_BORDER, r = blockIdx.y + SIFT_BORDER;
    const int img = blockIdx.z / nl, l0 = blockIdx.z % nl + 1;
    if (c >= w - SIFT_BORDER || r >= h - SIFT_BORDER)
        return;
    const float *__restrict__ D = dog_all + img * g.d_img + g.doff[o];
    const size_t plane = (size_t)w * h;
    const float *p = D + (size_t)l0 * plane + (size_t)r * w + c;
    const float val = *p;
    if (!(fabsf(val) > thr))
        return;
    bool ismax = val > 0.f, ismin = val < 0.f;
    for (int dl = -1; dl <= 1; dl++)
        for (int dr = -1; dr <= 1; dr++)
#pragma unroll
            for (int dc = -1; dc <= 1; dc++) {
                const float nb = p[(long long)dl * (long long)plane + dr * w + dc];
                ismax = ismax && val >= nb;
                ismin = ismin && val <= nb;
            }
    if (!(ismax || ismin))
        return;
    int l = l0, rr = r, cc = c;
    for (int it = 0; it < SIFT_STEPS; it++) {
        const SiftDeriv d = sift_derivs(D, w, plane, l, rr, cc);
        float xi, xr, xc;
        sift_solve(d, xi, xr, xc);
        if (fabsf(xi) < 0.5f && fabsf(xr) < 0.5f && fabsf(xc) < 0.5f) {
            if (sift_accept(d, xi, xr, xc, nl, cthr, ethr, nullptr))
                flags_all[(size_t)img * g.cells_img + g.coff[o] + ((size_t)(l - 1) * h + rr) * w + cc] = 1;
            return;
        }
        const float big = (float)(2147483647 / 3);
        if (!(fabsf(xi) <= big && fabsf(xr) <= big && fabsf(xc) <= big))
            return;
        cc += (int)__builtin_rintf(xc);
        rr += (int)__builtin_rintf(xr);
        l += (int)__builtin_rintf(xi);
        if (l < 1 || l > nl || cc < SIFT_BORDER || cc >= w - SIFT_BORDER || rr < SIFT_BORDER || rr >= h - SIFT_BORDER)
            return;
    }
}

// ---- 3. ordered compaction: block sums, scan of the sums, emit (the block scans are scan_ops.hip.h's) ----
template <class In> __global__ __launch_bounds__(SCAN_T) void scan_sums_kernel(In in, unsigned *__restrict__ bsum, int nblk)
{
    __shared__ unsigned s_wave[SCAN_T / 64];
    const int img = blockIdx.y, n = in.count(img);
    const int base = blockIdx.x * SCAN_BLOCK + threadIdx.x * SCAN_ITEMS;
    unsigned s = 0;
    for (int k = 0; k < SCAN_ITEMS; k++)
        if (base + k < n)
            s += in.get(img, base + k);
    unsigned total;
    svo::waves_before<SCAN_T>(svo::wave_sum(s), s_wave, &total);   // only the block's total
    if (threadIdx.x == 0)
        bsum[(size_t)img * nblk + blockIdx.x] = total;
}

// one workgroup per image: the block sums become exclusive offsets, the total goes to total[img]
__global__ __launch_bounds__(SCAN_T) void scan_offsets_kernel(unsigned *__restrict__ bsum, int nblk, int *__restrict__ total)
{
    __shared__ unsigned s_wave[SCAN_T / 64];
    unsigned *b = bsum + (size_t)blockIdx.x * nblk;
    const int per = (nblk + SCAN_T - 1) / SCAN_T, lo = threadIdx.x * per, hi = lo + per < nblk ? lo + per : nblk;
    unsigned s = 0;
    for (int i = lo; i < hi; i++)
        s += b[i];
    unsigned tot;
    unsigned run = svo::block_excl_scan<SCAN_T>(s, s_wave, &tot);
    for (int i = lo; i < hi; i++) {
        const unsigned v = b[i];
        b[i] = run;
        run += v;
    }
    if (threadIdx.x == 0)
        total[blockIdx.x] = (int)tot;
}

template <class In, class Emit>
__global__ __launch_bounds__(SCAN_T) void scan_emit_kernel(In in, const unsigned *__restrict__ bsum, int nblk, Emit emit)
{
    __shared__ unsigned s_wave[SCAN_T / 64];
    const int img = blockIdx.y, n = in.count(img);
    const int base = blockIdx.x * SCAN_BLOCK + threadIdx.x * SCAN_ITEMS;
    unsigned v[SCAN_ITEMS], s = 0;
    for (int k = 0; k < SCAN_ITEMS; k++) {
        v[k] = base + k < n ? in.get(img, base + k) : 0u;
        s += v[k];
    }
    unsigned pos = svo::block_excl_scan<SCAN_T>(s, s_wave, (unsigned *)nullptr) + bsum[(size_t)img * nblk + blockIdx.x];
    for (int k = 0; k < SCAN_ITEMS; k++)
        if (v[k]) {
            emit(img, base + k, pos, v[k]);
            pos += v[k];
        }
}

struct FlagsIn {
    const uint8_t *f;
    int stride, n;
    __device__ int count(int) const { return n; }
    __device__ unsigned get(int img, int i) const { return f[(size_t)img * stride + i]; }
};
struct CellEmit {
    unsigned *cells;
    __device__ void operator()(int img, int i, unsigned pos, unsigned) const
    {
        if (pos < (unsigned)SIFT_KP_CAP)
            cells[(size_t)img * SIFT_KP_CAP + pos] = (unsigned)i;
    }
};

// the key points of the refined cells (before orientation), per image SIFT_KP_CAP entries
struct SiftCellKp {
    float *x, *y, *size, *resp, *ang;   // ang: SIFT_MAXPEAK per cell
    int *oct;
    uint8_t *cnt;
};
// oriented key points before retainBest, per image SIFT_ORI_CAP entries
struct SiftOriKp {
    float *x, *y, *size, *resp, *ang;
    int *oct;
};

struct CountIn {
    const uint8_t *cnt;
    const int *d_n;
    __device__ int count(int img) const { return d_n[img] < SIFT_KP_CAP ? d_n[img] : SIFT_KP_CAP; }
    __device__ unsigned get(int img, int i) const { return cnt[(size_t)img * SIFT_KP_CAP + i]; }
};
struct OriEmit {
    SiftCellKp a;
    SiftOriKp b;
    __device__ void operator()(int img, int i, unsigned pos, unsigned v) const
    {
        const size_t s = (size_t)img * SIFT_KP_CAP + i;
        for (unsigned k = 0; k < v; k++) {
            if (pos + k >= (unsigned)SIFT_ORI_CAP)
                return;
            const size_t d = (size_t)img * SIFT_ORI_CAP + pos + k;
            b.x[d] = a.x[s];
            b.y[d] = a.y[s];
            b.size[d] = a.size[s];
            b.resp[d] = a.resp[s];
            b.oct[d] = a.oct[s];
            b.ang[d] = a.ang[s * SIFT_MAXPEAK + k];
        }
    }
};

struct KeepIn {
    const float *resp;
    const int *d_n;
    const unsigned *thr;
    __device__ int count(int img) const { return d_n[img] < SIFT_ORI_CAP ? d_n[img] : SIFT_ORI_CAP; }
    __device__ unsigned get(int img, int i) const
    {
        return __float_as_uint(resp[(size_t)img * SIFT_ORI_CAP + i]) >= thr[img] ? 1u : 0u;
    }
};
struct SiftOut {
    float *xy, *size, *angle, *resp;
    int *oct;
    int cap;
};
struct FinalEmit {
    SiftOriKp b;
    SiftOut o;
    __device__ void operator()(int img, int i, unsigned pos, unsigned) const
    {
        if (pos >= (unsigned)o.cap)
            return;
        const size_t s = (size_t)img * SIFT_ORI_CAP + i, d = (size_t)img * o.cap + pos;
        // the doubled first octave: octave - 1 in the low byte, pt and size halved
        o.xy[2 * d] = b.x[s] * 0.5f;
        o.xy[2 * d + 1] = b.y[s] * 0.5f;
        o.size[d] = b.size[s] * 0.5f;
        o.angle[d] = b.ang[s];
        o.resp[d] = b.resp[s];
        const int oc = b.oct[s];
        o.oct[d] = (oc & ~255) | ((oc - 1) & 255);
    }
};

// ---- 4. orientation: one wavefront (= one workgroup) per refined cell; grid (SIFT_KP_CAP, batch) ----
__global__ __launch_bounds__(64) void sift_orient_kernel(SiftGeom g, const float *__restrict__ gauss_all,
                                                         const float *__restrict__ dog_all, const unsigned *__restrict__ cells,
                                                         const int *__restrict__ d_ncell, float sigma, float cthr, float ethr,
                                                         SiftCellKp kp)
{
    __shared__ unsigned long long q[SIFT_ORI_BINS];
    __shared__ float th[SIFT_ORI_BINS], hs[SIFT_ORI_BINS];
    const int img = blockIdx.y, lane = threadIdx.x;
    const int ncell = d_ncell[img] < SIFT_KP_CAP ? d_ncell[img] : SIFT_KP_CAP;
    if ((int)blockIdx.x >= ncell)
        return;
    const size_t slot = (size_t)img * SIFT_KP_CAP + blockIdx.x;
    const int idx = (int)cells[slot];
    int o = 0;
    while (o + 1 < g.no && idx >= g.coff[o + 1])
        o++;
    const int w = g.w[o], h = g.h[o], nl = g.nl;
    const int rem = idx - g.coff[o], l = rem / (w * h) + 1, r = (rem % (w * h)) / w, c = rem % w;
    const size_t plane = (size_t)w * h;
    const SiftDeriv d = sift_derivs(dog_all + img * g.d_img + g.doff[o], w, plane, l, r, c);
    float xi, xr, xc, contr;
    sift_solve(d, xi, xr, xc);
    sift_accept(d, xi, xr, xc, nl, cthr, ethr, &contr);
    const float po = (float)(1 << o);
    const float t = ((float)l + xi) / (float)nl;
    const float size = sigma * (float)svo_exp((double)t * SIFT_LN2) * po * 2.f;
    const float scl = size * 0.5f / po;
    const int radius = (int)__builtin_rintf(4.5f * scl);
    const float sg = 1.5f * scl, expf_scale = -1.f / (2.f * sg * sg);
    if (lane < SIFT_ORI_BINS)
        q[lane] = 0ull;
    __syncthreads();
    const float *__restrict__ im = gauss_all + img * g.g_img + g.goff[o] + (size_t)l * plane;
    // rows r + i in [1, h - 2], columns c + j in [1, w - 2]
    const int ilo = -radius > 1 - r ? -radius : 1 - r, ihi = radius < h - 2 - r ? radius : h - 2 - r;
    const int jlo = -radius > 1 - c ? -radius : 1 - c, jhi = radius < w - 2 - c ? radius : w - 2 - c;
    const int nj = jhi - jlo + 1, ns = (ihi >= ilo && nj > 0) ? (ihi - ilo + 1) * nj : 0;
    for (int s = lane; s < ns; s += 64) {
        const int i = ilo + s / nj, j = jlo + s % nj;
        const float *p = im + (size_t)(r + i) * w + (c + j);
        const float dx = p[1] - p[-1], dy = p[-w] - p[w];
        const float wt = (float)svo_exp((double)((float)(i * i + j * j) * expf_scale));
        const float ori = fast_atan2_deg(dy, dx), mag = sqrtf(dx * dx + dy * dy);
        int bin = (int)__builtin_rintf((36.f / 360.f) * ori);
        if (bin >= SIFT_ORI_BINS)
            bin -= SIFT_ORI_BINS;
        if (bin < 0)
            bin += SIFT_ORI_BINS;
        const long long qv = (long long)__builtin_rint((double)(wt * mag) * SIFT_Q);
        atomicAdd(&q[bin], (unsigned long long)qv);
    }
    __syncthreads();
    if (lane < SIFT_ORI_BINS)
        th[lane] = (float)((double)(long long)q[lane] * SIFT_QINV);
    __syncthreads();
    if (lane < SIFT_ORI_BINS) {
        const int n = SIFT_ORI_BINS;
        hs[lane] = (th[(lane + n - 2) % n] + th[(lane + 2) % n]) * (1.f / 16.f) +
                   (th[(lane + n - 1) % n] + th[(lane + 1) % n]) * (4.f / 16.f) + th[lane] * (6.f / 16.f);
    }
    __syncthreads();
    float mx = hs[0];
    for (int k = 1; k < SIFT_ORI_BINS; k++)
        mx = fmaxf(mx, hs[k]);
    const float mag_thr = mx * 0.8f;
    bool peak = false;
    float ang = 0.f;
    if (lane < SIFT_ORI_BINS) {
        const int n = SIFT_ORI_BINS;
        const float hl = hs[(lane + n - 1) % n], hj = hs[lane], hr = hs[(lane + 1) % n];
        if (hj > hl && hj > hr && hj >= mag_thr) {
            peak = true;
            float bin = (float)lane + 0.5f * (hl - hr) / (hl - 2.f * hj + hr);
            bin = bin < 0.f ? (float)n + bin : (bin >= (float)n ? bin - (float)n : bin);
            ang = 360.f - (360.f / 36.f) * bin;
            if (fabsf(ang - 360.f) < 1.1920929e-07f)
                ang = 0.f;
        }
    }
    const unsigned long long m = __ballot(peak);
    if (peak) {
        const int rank = svo::lanes_below(m);
        if (rank < SIFT_MAXPEAK)
            kp.ang[slot * SIFT_MAXPEAK + rank] = ang;
    }
    if (lane == 0) {
        const int np = __popcll(m);
        kp.cnt[slot] = (uint8_t)(np < SIFT_MAXPEAK ? np : SIFT_MAXPEAK);
        kp.x[slot] = ((float)c + xc) * po;
        kp.y[slot] = ((float)r + xr) * po;
        kp.size[slot] = size;
        kp.resp[slot] = fabsf(contr);
        kp.oct[slot] = o + (l << 8) + ((int)__builtin_rint(((double)xi + 0.5) * 255) << 16);
    }
}

// ---- 5. retainBest: the n-th largest response by radix selection, one workgroup per image ----
__global__ __launch_bounds__(1024) void sift_select_kernel(const float *__restrict__ resp_all, const int *__restrict__ d_n,
                                                           int n_features, unsigned *__restrict__ thr)
{
    __shared__ unsigned hist[256];
    __shared__ unsigned s_prefix;
    __shared__ int s_k;
    const int img = blockIdx.x, n = d_n[img] < SIFT_ORI_CAP ? d_n[img] : SIFT_ORI_CAP;
    if (n_features <= 0 || n <= n_features) {   // uniform over the workgroup
        if (threadIdx.x == 0)
            thr[img] = 0u;
        return;
    }
    const float *__restrict__ resp = resp_all + (size_t)img * SIFT_ORI_CAP;
    unsigned prefix = 0, mask = 0;
    int k = n_features;
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (threadIdx.x < 256)
            hist[threadIdx.x] = 0;
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += 1024) {
            const unsigned b = __float_as_uint(resp[i]);
            if ((b & mask) == prefix)
                atomicAdd(&hist[(b >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            int cum = 0, dsel = 0;
            for (int dgt = 255; dgt >= 0; dgt--) {
                if (cum + (int)hist[dgt] >= k) {
                    dsel = dgt;
                    break;
                }
                cum += (int)hist[dgt];
            }
            s_prefix = prefix | ((unsigned)dsel << shift);
            s_k = k - cum;
        }
        __syncthreads();
        prefix = s_prefix;
        k = s_k;
        mask |= 0xffu << shift;
        __syncthreads();
    }
    if (threadIdx.x == 0)
        thr[img] = prefix;
}

// ---- 6. descriptors: one wavefront per key point; grid (cap, batch); d_n: live count per image (null: n_fixed) ----
__global__ __launch_bounds__(64) void sift_describe_kernel(SiftGeom g, const float *__restrict__ gauss_all,
                                                           const float *__restrict__ xy_all, const float *__restrict__ size_all,
                                                           const float *__restrict__ angle_all, const int *__restrict__ oct_all,
                                                           const int *__restrict__ d_n, int n_fixed, int cap,
                                                           float *__restrict__ desc_all)
{
    constexpr int D = 4, N = 8, HL = (D + 2) * (D + 2) * (N + 2);
    __shared__ unsigned long long q[HL];
    __shared__ float hf[HL], dst[D * D * N];
    const int img = blockIdx.y, lane = threadIdx.x;
    int n = d_n ? d_n[img] : n_fixed;
    n = n < cap ? n : cap;
    if ((int)blockIdx.x >= n)
        return;
    const size_t slot = (size_t)img * cap + blockIdx.x;
    float *__restrict__ out = desc_all + slot * 128;
    const int packed = oct_all[slot];
    int o = packed & 255;
    const int layer = (packed >> 8) & 255;
    o = o < 128 ? o : (-128 | o);
    const float kx = xy_all[2 * slot], ky = xy_all[2 * slot + 1], ksz = size_all[slot];
    // key points that name no layer of this pyramid, or lie absurdly far outside it, get a zero descriptor
    const bool sane = o >= -1 && o + 1 < g.no && layer <= g.nl + 2 && fabsf(kx) < 1e8f && fabsf(ky) < 1e8f && ksz >= 0.f &&
                      ksz < 1e8f;
    if (!sane) {
        out[lane] = 0.f;
        out[lane + 64] = 0.f;
        return;
    }
    const float scale = o >= 0 ? 1.f / (float)(1 << o) : (float)(1 << -o);
    const int w = g.w[o + 1], h = g.h[o + 1];
    const float *__restrict__ im = gauss_all + img * g.g_img + g.goff[o + 1] + (size_t)layer * w * h;
    float ori = 360.f - angle_all[slot];
    if (fabsf(ori - 360.f) < 1.1920929e-07f)
        ori = 0.f;
    const float ptx = kx * scale, pty = ky * scale, scl = ksz * scale * 0.5f;
    const int px = (int)__builtin_rintf(ptx), py = (int)__builtin_rintf(pty);
    const float a = ori * (float)(3.14159265358979323846 / 180);
    float cos_t = (float)svo_cos((double)a), sin_t = (float)svo_sin((double)a);
    const float bins_per_rad = 8.f / 360.f, exp_scale = -1.f / (16.f * 0.5f), hist_width = 3.f * scl;
    int radius = (int)__builtin_rintf(hist_width * 1.4142135623730951f * 5.f * 0.5f);
    const int diag = (int)__builtin_sqrt((double)w * w + (double)h * h);
    radius = radius < diag ? radius : diag;
    cos_t = cos_t / hist_width;
    sin_t = sin_t / hist_width;
    for (int k = lane; k < HL; k += 64)
        q[k] = 0ull;
    __syncthreads();
    const int ilo = -radius > 1 - py ? -radius : 1 - py, ihi = radius < h - 2 - py ? radius : h - 2 - py;
    const int jlo = -radius > 1 - px ? -radius : 1 - px, jhi = radius < w - 2 - px ? radius : w - 2 - px;
    const int nj = jhi - jlo + 1, ns = (ihi >= ilo && nj > 0) ? (ihi - ilo + 1) * nj : 0;
    for (int s = lane; s < ns; s += 64) {
        const int i = ilo + s / nj, j = jlo + s % nj;
        const float fi = (float)i, fj = (float)j;
        const float c_rot = fj * cos_t - fi * sin_t, r_rot = fj * sin_t + fi * cos_t;
        float rbin = r_rot + 2.f - 0.5f, cbin = c_rot + 2.f - 0.5f;
        if (!(rbin > -1.f && rbin < (float)D && cbin > -1.f && cbin < (float)D))
            continue;
        const float *p = im + (size_t)(py + i) * w + (px + j);
        const float dx = p[1] - p[-1], dy = p[-w] - p[w];
        const float wt = (float)svo_exp((double)((c_rot * c_rot + r_rot * r_rot) * exp_scale));
        float obin = (fast_atan2_deg(dy, dx) - ori) * bins_per_rad;
        const float mag = sqrtf(dx * dx + dy * dy) * wt;
        const float fr0 = floorf(rbin), fc0 = floorf(cbin), fo0 = floorf(obin);
        rbin = rbin - fr0;
        cbin = cbin - fc0;
        obin = obin - fo0;
        const int r0 = (int)fr0, c0 = (int)fc0;
        int o0 = (int)fo0;
        if (o0 < 0)
            o0 += N;
        if (o0 >= N)
            o0 -= N;
        const float v_r1 = mag * rbin, v_r0 = mag - v_r1;
        const float v_rc11 = v_r1 * cbin, v_rc10 = v_r1 - v_rc11;
        const float v_rc01 = v_r0 * cbin, v_rc00 = v_r0 - v_rc01;
        const float v111 = v_rc11 * obin, v110 = v_rc11 - v111;
        const float v101 = v_rc10 * obin, v100 = v_rc10 - v101;
        const float v011 = v_rc01 * obin, v010 = v_rc01 - v011;
        const float v001 = v_rc00 * obin, v000 = v_rc00 - v001;
        const int idx = ((r0 + 1) * (D + 2) + c0 + 1) * (N + 2) + o0;
        constexpr int S = N + 2, T = (D + 2) * (N + 2);
        auto add = [&](int k, float v) {
            atomicAdd(&q[k], (unsigned long long)(long long)__builtin_rint((double)v * SIFT_Q));
        };
        add(idx, v000);
        add(idx + 1, v001);
        add(idx + S, v010);
        add(idx + S + 1, v011);
        add(idx + T, v100);
        add(idx + T + 1, v101);
        add(idx + T + S, v110);
        add(idx + T + S + 1, v111);
    }
    __syncthreads();
    for (int k = lane; k < HL; k += 64)
        hf[k] = (float)((double)(long long)q[k] * SIFT_QINV);
    __syncthreads();
    // the circular orientation bins: 8 -> 0, 9 -> 1
    for (int k = lane; k < 2 * D * D; k += 64) {
        const int cell = k >> 1, i = cell / D, j = cell % D, idx = ((i + 1) * (D + 2) + (j + 1)) * (N + 2) + (k & 1);
        hf[idx] = hf[idx] + hf[idx + N];
    }
    __syncthreads();
    for (int k = lane; k < D * D * N; k += 64) {
        const int cell = k / N, i = cell / D, j = cell % D;
        dst[k] = hf[((i + 1) * (D + 2) + (j + 1)) * (N + 2) + k % N];
    }
    __syncthreads();
    float nrm2 = 0.f;
    for (int k = 0; k < D * D * N; k++)
        nrm2 = nrm2 + dst[k] * dst[k];
    const float thr = sqrtf(nrm2) * 0.2f;
    nrm2 = 0.f;
    for (int k = 0; k < D * D * N; k++) {
        const float v = fminf(dst[k], thr);
        nrm2 = nrm2 + v * v;
    }
    const float s = 512.f / fmaxf(sqrtf(nrm2), 1.1920929e-07f);
    for (int k = lane; k < D * D * N; k += 64) {
        float v = __builtin_rintf(fminf(dst[k], thr) * s);
        v = v < 0.f ? 0.f : (v > 255.f ? 255.f : v);
        out[k] = v;
    }
}

// ---- host side ----
struct SiftPlan {
    SiftGeom g;
    int w, h, c, B;
    float thr, cthr, ethr, sigma;
    int ks[12];            // kernel sizes: [0] the initial blur, [i] layer i
    SiftTaps taps[12];
    float *gauss, *dog, *base, *tmp;
    long long base_img;    // floats per image of base / tmp (the doubled frame)
    uint8_t *flags;
    unsigned *bsum, *cells, *thr_bits;
    int nblk_cells;
    int *counts;           // [3][B]: cells, oriented, kept
    SiftCellKp ckp;
    SiftOriKp okp;
};

int sift_gauss_kernel(double sigma, float *cf)
{
    const int n = (int)std::rint(sigma * 8 + 1) | 1;
    if (n > SIFT_KSTRIDE - 1)
        return -1;
    const double s2x = -0.5 / (sigma * sigma);
    for (int i = 0; i < n; i++) {
        const double x = i - (n - 1) * 0.5;
        cf[i] = (float)svo_exp(s2x * x * x);
    }
    double sum = 0;
    for (int i = 0; i < n; i++)
        sum += cf[i];
    sum = 1.0 / sum;
    for (int i = 0; i < n; i++)
        cf[i] = (float)(cf[i] * sum);
    return n;
}

int sift_check_params(const svo_sift_params *prm, svo_sift_params &p, int w, int h, int c)
{
    if (prm)
        p = *prm;
    else
        svo_sift_default_params(&p);
    SVO_CHECK_ARG(c == 1 || c == 3);
    SVO_CHECK_ARG(p.n_octave_layers >= 1 && p.n_octave_layers <= 8 && p.n_features >= 0);
    SVO_CHECK_ARG(p.sigma > 0 && p.contrast_threshold >= 0 && p.edge_threshold >= 0);
    // the smallest frame the recipe gives an octave: cvRound(log2(2 min(w, h)) - 2) + 1 >= 1
    SVO_CHECK_ARG(w >= 2 && h >= 2 && w <= 16384 && h <= 16384);
    return SVO_OK;
}

int sift_plan(svo_ctx *ctx, int w, int h, int c, const svo_sift_params &p, int B, SiftPlan &pl)
{
    SiftGeom &g = pl.g;
    pl.w = w;
    pl.h = h;
    pl.c = c;
    pl.B = B;
    const int nl = p.n_octave_layers;
    g.nl = nl;
    const int m = 2 * (w < h ? w : h);
    g.no = (int)std::rint(std::log((double)m) / std::log(2.0) - 2) + 1;
    SVO_CHECK_ARG(g.no >= 1 && g.no <= SIFT_MAXOCT);
    long long go = 0, dof = 0, co = 0;
    for (int o = 0; o < g.no; o++) {
        g.w[o] = o ? g.w[o - 1] / 2 : 2 * w;
        g.h[o] = o ? g.h[o - 1] / 2 : 2 * h;
        SVO_CHECK_ARG(g.w[o] >= 1 && g.h[o] >= 1);
        const long long px = (long long)g.w[o] * g.h[o];
        g.goff[o] = go;
        g.doff[o] = dof;
        g.coff[o] = (int)co;
        go += px * (nl + 3);
        dof += px * (nl + 2);
        co += px * nl;
        if (co >= (1ll << 31) - 2 * SCAN_BLOCK) {
            svo_set_error("svo_sift: %d x %d with %d layers has more than 2^31 scale-space cells", w, h, nl);
            return SVO_ERR_CAPACITY;
        }
    }
    for (int o = g.no; o <= SIFT_MAXOCT; o++)
        g.coff[o] = (int)co;
    g.g_img = (go + 63) & ~63ll;
    g.d_img = (dof + 63) & ~63ll;
    g.cells_img = (int)((co + 15) & ~15ll);
    pl.thr = (float)(int)std::floor(0.5 * p.contrast_threshold / nl * 255);
    pl.cthr = (float)p.contrast_threshold;
    pl.ethr = (float)p.edge_threshold;
    pl.sigma = (float)p.sigma;
    // the Gaussian kernels: [0] the blur of the doubled frame, [i] the step to layer i
    memset(pl.taps, 0, sizeof(pl.taps));
    const float sf = (float)p.sigma;
    const float sig_diff = sqrtf(std::fmax(sf * sf - 0.5f * 0.5f * 4, 0.01f));
    double sig[12];
    sig[0] = sig_diff;
    {
        const double k = svo_exp(SIFT_LN2 / nl);
        double pw = 1.0;
        for (int i = 1; i < nl + 3; i++) {
            const double prev = pw * p.sigma, total = prev * k;
            sig[i] = std::sqrt(total * total - prev * prev);
            pw = pw * k;
        }
    }
    for (int i = 0; i < nl + 3; i++) {
        pl.ks[i] = sift_gauss_kernel(sig[i], pl.taps[i].k);
        if (pl.ks[i] < 0) {
            svo_set_error("svo_sift: sigma %g needs a Gaussian kernel of more than %d taps", p.sigma, SIFT_KSTRIDE - 1);
            return SVO_ERR_ARG;
        }
    }
    pl.base_img = ((long long)4 * w * h + 63) & ~63ll;
    pl.nblk_cells = (g.cells_img + SCAN_BLOCK - 1) / SCAN_BLOCK;
    int rc;
    if ((rc = ctx->sift_pyr.ensure(((size_t)g.g_img + g.d_img + 2 * pl.base_img) * 4 * B + 1024)))
        return rc;
    uint8_t *q = ctx->sift_pyr.as<uint8_t>();
    pl.gauss = bump<float>(q, (size_t)g.g_img * B);
    pl.dog = bump<float>(q, (size_t)g.d_img * B);
    pl.base = bump<float>(q, (size_t)pl.base_img * B);
    pl.tmp = bump<float>(q, (size_t)pl.base_img * B);
    const size_t nb_scan = (size_t)(pl.nblk_cells > (SIFT_ORI_CAP / SCAN_BLOCK) ? pl.nblk_cells : SIFT_ORI_CAP / SCAN_BLOCK) + 1;
    const size_t work = (size_t)B * g.cells_img + nb_scan * B * 4 + (size_t)B * SIFT_KP_CAP * 4 +
                        (size_t)B * 64 + (size_t)B * SIFT_KP_CAP * (4 * 4 + 4 + 1 + 4 * SIFT_MAXPEAK) +
                        (size_t)B * SIFT_ORI_CAP * 6 * 4 + 32 * 256;
    if ((rc = ctx->sift_work.ensure(work)))
        return rc;
    q = ctx->sift_work.as<uint8_t>();
    pl.flags = bump<uint8_t>(q, (size_t)B * g.cells_img);
    pl.bsum = bump<unsigned>(q, nb_scan * B);
    pl.cells = bump<unsigned>(q, (size_t)B * SIFT_KP_CAP);
    pl.thr_bits = bump<unsigned>(q, B);
    pl.counts = bump<int>(q, 3 * B);
    const size_t nk = (size_t)B * SIFT_KP_CAP, no = (size_t)B * SIFT_ORI_CAP;
    pl.ckp.x = bump<float>(q, nk);
    pl.ckp.y = bump<float>(q, nk);
    pl.ckp.size = bump<float>(q, nk);
    pl.ckp.resp = bump<float>(q, nk);
    pl.ckp.oct = bump<int>(q, nk);
    pl.ckp.cnt = bump<uint8_t>(q, nk);
    pl.ckp.ang = bump<float>(q, nk * SIFT_MAXPEAK);
    pl.okp.x = bump<float>(q, no);
    pl.okp.y = bump<float>(q, no);
    pl.okp.size = bump<float>(q, no);
    pl.okp.resp = bump<float>(q, no);
    pl.okp.ang = bump<float>(q, no);
    pl.okp.oct = bump<int>(q, no);
    return SVO_OK;
}

// the scale space of nb device images
int sift_build_pyramids(svo_ctx *ctx, const SiftPlan &pl, const uint8_t *const *d_images, int nb)
{
    hipStream_t st = ctx->stream;
    const SiftGeom &g = pl.g;
    const int W = g.w[0], H = g.h[0];
    hipLaunchKernelGGL(sift_init_kernel, dim3((W + 255) / 256, H, nb), dim3(256), 0, st, make_image_batch(d_images, nb), pl.w, pl.h, pl.c,
                       pl.base, pl.base_img);
    for (int o = 0; o < g.no; o++) {
        const int w = g.w[o], h = g.h[o];
        const long long px = (long long)w * h;
        const dim3 grid((w + 255) / 256, h, nb);
        float *G = pl.gauss + g.goff[o], *Dg = pl.dog + g.doff[o];
        if (o == 0) {
            hipLaunchKernelGGL(sift_blur_row_kernel, grid, dim3(256), 0, st, pl.base, pl.base_img, pl.tmp, pl.base_img, w, h,
                               pl.taps[0], pl.ks[0]);
            hipLaunchKernelGGL(sift_blur_col_kernel, grid, dim3(256), 0, st, pl.tmp, pl.base_img, G, (const float *)nullptr,
                               g.g_img, (float *)nullptr, g.d_img, w, h, pl.taps[0], pl.ks[0]);
        } else {
            hipLaunchKernelGGL(sift_decimate_kernel, grid, dim3(256), 0, st, pl.gauss + g.goff[o - 1] + (long long)g.nl * g.w[o - 1] * g.h[o - 1],
                               G, g.g_img, g.w[o - 1], w, h);
        }
        for (int i = 1; i < g.nl + 3; i++) {
            const SiftTaps &k = pl.taps[i];
            hipLaunchKernelGGL(sift_blur_row_kernel, grid, dim3(256), 0, st, G + (i - 1) * px, g.g_img, pl.tmp, pl.base_img, w, h, k,
                               pl.ks[i]);
            hipLaunchKernelGGL(sift_blur_col_kernel, grid, dim3(256), 0, st, pl.tmp, pl.base_img, G + i * px, G + (i - 1) * px, g.g_img,
                               Dg + (i - 1) * px, g.d_img, w, h, k, pl.ks[i]);
        }
    }
    SVO_HIP(hipGetLastError());
    return SVO_OK;
}

// detection (+ descriptors) of nb images whose scale space stands; outputs: device arrays of nb x cap entries
int sift_detect(svo_ctx *ctx, const SiftPlan &pl, int nb, int n_features, const SiftOut &out, float *d_desc)
{
    hipStream_t st = ctx->stream;
    const SiftGeom &g = pl.g;
    SVO_HIP(hipMemsetAsync(pl.flags, 0, (size_t)nb * g.cells_img, st));
    for (int o = 0; o < g.no; o++) {
        const int w = g.w[o], h = g.h[o];
        if (w <= 2 * SIFT_BORDER || h <= 2 * SIFT_BORDER)
            continue;
        hipLaunchKernelGGL(sift_extrema_kernel, dim3((w - 2 * SIFT_BORDER + 255) / 256, h - 2 * SIFT_BORDER, nb * g.nl), dim3(256), 0,
                           st, g, o, pl.dog, pl.flags, pl.thr, pl.cthr, pl.ethr);
    }
    int *n_cell = pl.counts, *n_ori = pl.counts + pl.B, *n_keep = pl.counts + 2 * pl.B;
    {
        const FlagsIn in{pl.flags, g.cells_img, g.cells_img};
        const int nblk = pl.nblk_cells;
        hipLaunchKernelGGL(scan_sums_kernel<FlagsIn>, dim3(nblk, nb), dim3(SCAN_T), 0, st, in, pl.bsum, nblk);
        hipLaunchKernelGGL(scan_offsets_kernel, dim3(nb), dim3(SCAN_T), 0, st, pl.bsum, nblk, n_cell);
        hipLaunchKernelGGL((scan_emit_kernel<FlagsIn, CellEmit>), dim3(nblk, nb), dim3(SCAN_T), 0, st, in, pl.bsum, nblk,
                           CellEmit{pl.cells});
    }
    hipLaunchKernelGGL(sift_orient_kernel, dim3(SIFT_KP_CAP, nb), dim3(64), 0, st, g, pl.gauss, pl.dog, pl.cells, n_cell, pl.sigma,
                       pl.cthr, pl.ethr, pl.ckp);
    {
        const CountIn in{pl.ckp.cnt, n_cell};
        const int nblk = SIFT_KP_CAP / SCAN_BLOCK;
        hipLaunchKernelGGL(scan_sums_kernel<CountIn>, dim3(nblk, nb), dim3(SCAN_T), 0, st, in, pl.bsum, nblk);
        hipLaunchKernelGGL(scan_offsets_kernel, dim3(nb), dim3(SCAN_T), 0, st, pl.bsum, nblk, n_ori);
        hipLaunchKernelGGL((scan_emit_kernel<CountIn, OriEmit>), dim3(nblk, nb), dim3(SCAN_T), 0, st, in, pl.bsum, nblk,
                           OriEmit{pl.ckp, pl.okp});
    }
    hipLaunchKernelGGL(sift_select_kernel, dim3(nb), dim3(1024), 0, st, pl.okp.resp, n_ori, n_features, pl.thr_bits);
    {
        const KeepIn in{pl.okp.resp, n_ori, pl.thr_bits};
        const int nblk = SIFT_ORI_CAP / SCAN_BLOCK;
        hipLaunchKernelGGL(scan_sums_kernel<KeepIn>, dim3(nblk, nb), dim3(SCAN_T), 0, st, in, pl.bsum, nblk);
        hipLaunchKernelGGL(scan_offsets_kernel, dim3(nb), dim3(SCAN_T), 0, st, pl.bsum, nblk, n_keep);
        hipLaunchKernelGGL((scan_emit_kernel<KeepIn, FinalEmit>), dim3(nblk, nb), dim3(SCAN_T), 0, st, in, pl.bsum, nblk,
                           FinalEmit{pl.okp, out});
    }
    if (d_desc) {
        const int gx = out.cap < SIFT_ORI_CAP ? out.cap : SIFT_ORI_CAP;
        hipLaunchKernelGGL(sift_describe_kernel, dim3(gx, nb), dim3(64), 0, st, g, pl.gauss, out.xy, out.size, out.angle, out.oct,
                           n_keep, 0, out.cap, d_desc);
    }
    SVO_HIP(hipGetLastError());
    return SVO_OK;
}

}  // namespace

extern "C" {

void svo_sift_default_params(svo_sift_params *p)
{
    if (!p)
        return;
    p->n_features = 0;   // SIFT::create()
    p->n_octave_layers = 3;
    p->contrast_threshold = 0.04;
    p->edge_threshold = 10;
    p->sigma = 1.6;
}

int svo_sift_extract_batch(svo_ctx *ctx, const uint8_t *const *images, int n_images, int w, int h, int c,
                           const svo_sift_params *prm, int cap, float *xy, float *size, float *angle, float *response, int *octave,
                           float *desc, int *n, int mem)
{
    SVO_CHECK_ARG(ctx && images && n && xy && size && angle && response && octave);
    SVO_CHECK_ARG(n_images >= 1 && n_images <= SIFT_MAXBATCH && cap >= 1);
    SVO_CHECK_ARG(mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE);
    SVO_CHECK_ARG(aligned4(xy) && aligned4(size) && aligned4(angle) && aligned4(response) && aligned4(octave) && aligned4(desc) &&
                  aligned4(n));
    for (int k = 0; k < n_images; k++)
        SVO_CHECK_ARG(images[k] != nullptr);
    svo_sift_params p;
    int rc;
    if ((rc = sift_check_params(prm, p, w, h, c)))
        return rc;
    SVO_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    SiftPlan pl;
    if ((rc = sift_plan(ctx, w, h, c, p, n_images, pl)))
        return rc;
    const size_t e = (size_t)n_images * cap;
    const uint8_t *ptrs[SIFT_MAXBATCH];
    SiftOut out{xy, size, angle, response, octave, cap};
    float *d_desc = desc;
    if ((rc = stage_images(ctx, images, n_images, (size_t)w * h * c, mem, ptrs)))
        return rc;
    if (mem == SVO_MEM_HOST) {
        if ((rc = ctx->sift_out.ensure(e * (6 + (desc ? 128 : 0)) * 4 + 2048)))
            return rc;
        uint8_t *q = ctx->sift_out.as<uint8_t>();
        out.xy = bump<float>(q, 2 * e);
        out.size = bump<float>(q, e);
        out.angle = bump<float>(q, e);
        out.resp = bump<float>(q, e);
        out.oct = bump<int>(q, e);
        d_desc = desc ? bump<float>(q, 128 * e) : nullptr;
    }
    if ((rc = sift_build_pyramids(ctx, pl, ptrs, n_images)) || (rc = sift_detect(ctx, pl, n_images, p.n_features, out, d_desc)))
        return rc;
    // the one wait: the counts
    int counts[3 * SIFT_MAXBATCH];
    if ((rc = read_counts(ctx, pl.counts, 3 * n_images, counts)))
        return rc;
    for (int k = 0; k < n_images; k++) {
        const int nc = counts[k], no = counts[n_images + k], nk = counts[2 * n_images + k];
        n[k] = nk;
        if (nc > SIFT_KP_CAP || no > SIFT_ORI_CAP) {
            svo_set_error("svo_sift_extract_batch: image %d has %d extrema / %d oriented key points before the filters (the work "
                          "arrays hold %d / %d)", k, nc, no, SIFT_KP_CAP, SIFT_ORI_CAP);
            return SVO_ERR_CAPACITY;
        }
        if (nk > cap && rc == SVO_OK) {
            svo_set_error("svo_sift_extract_batch: image %d yields %d key points, cap is %d", k, nk, cap);
            rc = SVO_ERR_CAPACITY;
        }
    }
    if (mem == SVO_MEM_HOST) {
        const HostColumn cols[6] = {{xy, out.xy, 8},         {size, out.size, 4},  {angle, out.angle, 4},
                                    {response, out.resp, 4}, {octave, out.oct, 4}, {desc, d_desc, 128 * sizeof(float)}};
        const int rc_copy = copy_rows_to_host(st, cols, 6, n_images, cap, n);
        if (rc_copy)
            return rc_copy;
    }
    return rc;
}

int svo_sift_describe(svo_ctx *ctx, const uint8_t *image, int w, int h, int c, const svo_sift_params *prm, const float *xy,
                      const float *size, const float *angle, const int *octave, int n, float *desc, int mem)
{
    SVO_CHECK_ARG(ctx && image && n >= 0 && (n == 0 || (xy && size && angle && octave && desc)));
    SVO_CHECK_ARG(mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE);
    SVO_CHECK_ARG(aligned4(xy) && aligned4(size) && aligned4(angle) && aligned4(octave) && aligned4(desc));
    svo_sift_params p;
    int rc;
    if ((rc = sift_check_params(prm, p, w, h, c)))
        return rc;
    if (n == 0)
        return SVO_OK;
    SVO_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    SiftPlan pl;
    if ((rc = sift_plan(ctx, w, h, c, p, 1, pl)))
        return rc;
    const size_t e = (size_t)n;
    const uint8_t *d_img = nullptr;
    const float *dxy = xy, *dsize = size, *dang = angle;
    const int *doct = octave;
    float *ddesc = desc;
    if ((rc = stage_images(ctx, &image, 1, (size_t)w * h * c, mem, &d_img)))
        return rc;
    if (mem == SVO_MEM_HOST) {
        if ((rc = ctx->sift_out.ensure(e * (5 + 128) * 4 + 2048)))
            return rc;
        uint8_t *q = ctx->sift_out.as<uint8_t>();
        float *a = bump<float>(q, 2 * e), *b = bump<float>(q, e), *cc = bump<float>(q, e);
        int *d = bump<int>(q, e);
        ddesc = bump<float>(q, 128 * e);
        SVO_HIP(hipMemcpyAsync(a, xy, e * 8, hipMemcpyHostToDevice, st));
        SVO_HIP(hipMemcpyAsync(b, size, e * 4, hipMemcpyHostToDevice, st));
        SVO_HIP(hipMemcpyAsync(cc, angle, e * 4, hipMemcpyHostToDevice, st));
        SVO_HIP(hipMemcpyAsync(d, octave, e * 4, hipMemcpyHostToDevice, st));
        dxy = a;
        dsize = b;
        dang = cc;
        doct = d;
    }
    if ((rc = sift_build_pyramids(ctx, pl, &d_img, 1)))
        return rc;
    hipLaunchKernelGGL(sift_describe_kernel, dim3(n, 1), dim3(64), 0, st, pl.g, pl.gauss, dxy, dsize, dang, doct, (const int *)nullptr,
                       n, n, ddesc);
    SVO_HIP(hipGetLastError());
    if (mem == SVO_MEM_HOST) {
        SVO_HIP(hipMemcpyAsync(desc, ddesc, e * 512, hipMemcpyDeviceToHost, st));
        SVO_HIP(hipStreamSynchronize(st));
    }
    return SVO_OK;
}

int svo_sift_pyramid_layout(int w, int h, int n_octave_layers, int *n_octaves, int *ow, int *oh)
{
    SVO_CHECK_ARG(w >= 2 && h >= 2 && w <= 16384 && h <= 16384 && n_octave_layers >= 1 && n_octave_layers <= 8 && n_octaves);
    const int m = 2 * (w < h ? w : h);
    const int no = (int)std::rint(std::log((double)m) / std::log(2.0) - 2) + 1;
    SVO_CHECK_ARG(no >= 1 && no <= SIFT_MAXOCT);
    *n_octaves = no;
    for (int o = 0, cw = 2 * w, ch = 2 * h; o < no; o++, cw /= 2, ch /= 2) {
        if (ow)
            ow[o] = cw;
        if (oh)
            oh[o] = ch;
    }
    return SVO_OK;
}

int svo_sift_pyramid(svo_ctx *ctx, const uint8_t *image, int w, int h, int c, const svo_sift_params *prm, float *gauss, float *dog,
                     int mem)
{
    SVO_CHECK_ARG(ctx && image && gauss && dog && aligned4(gauss) && aligned4(dog));
    SVO_CHECK_ARG(mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE);
    svo_sift_params p;
    int rc;
    if ((rc = sift_check_params(prm, p, w, h, c)))
        return rc;
    SVO_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    SiftPlan pl;
    if ((rc = sift_plan(ctx, w, h, c, p, 1, pl)))
        return rc;
    const uint8_t *d_img = nullptr;
    if ((rc = stage_images(ctx, &image, 1, (size_t)w * h * c, mem, &d_img)) || (rc = sift_build_pyramids(ctx, pl, &d_img, 1)))
        return rc;
    const SiftGeom &g = pl.g;
    const int last = g.no - 1;
    const size_t ng = (size_t)g.goff[last] + (size_t)g.w[last] * g.h[last] * (g.nl + 3);
    const size_t nd = (size_t)g.doff[last] + (size_t)g.w[last] * g.h[last] * (g.nl + 2);
    const hipMemcpyKind kind = mem == SVO_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    SVO_HIP(hipMemcpyAsync(gauss, pl.gauss, ng * 4, kind, st));
    SVO_HIP(hipMemcpyAsync(dog, pl.dog, nd * 4, kind, st));
    if (mem == SVO_MEM_HOST)
        SVO_HIP(hipStreamSynchronize(st));
    return SVO_OK;
}

}  // extern "C"
