// wls.hip -- the disparity WLS filter the reference's author wrote around the matcher (src/StereoCV.cpp:25-28,51-59, commented
// out upstream): ximgproc::createDisparityWLSFilter(matcher), createRightMatcher(matcher), filter(disp, grey, out, rdisp).
// The recipe and every recalled or chosen point of it: tests/wls_numpy.py (W1..W6), DESIGN.md section 10h.  The float32
// operation order of W3..W6 is the contract: the results are bit-identical to the restatement.
//
// Per call (n pairs, blockIdx.y = pair; every plane below is n x ROI height x ROI width):
//   wls_box_h_kernel    one thread per ROI pixel of one view: the row sums of d and d^2 over 2r+1 reflected columns (integers)
//   wls_box_v_kernel    the column sums of those over 2r+1 reflected rows, the two means, dd = max(0, 1 - roll_off * var) (W3)
//   wls_conf_kernel     one thread per image pixel: the left-right check, conf = min(dd_l, dd_r) or 0 (W4), the planes
//                       num = d * conf and den = conf, the confidence map conf * 255 (zero outside the ROI)
//   wls_weights_kernel  Chor / Cvert from the guide through the table of -exp(-k / sigma) (W5)
//   wls_hsweep_kernel   one lane per row, 64 rows per wave: tiles of 64 rows x 32 columns go through LDS both ways, so global
//                       memory is read and written along rows while each lane walks its own row (row pitch 33 floats: the
//                       lane-per-row walk and the row-per-half-wave copy are both free of bank conflicts); forward pass tile by
//                       tile left to right (t kept in a plane of its own), backward pass right to left
//   wls_vsweep_kernel   one lane per column, serial down the column: every access is coalesced as it stands
//   wls_finish_kernel   one thread per image pixel: rint(num / (den + FLT_EPSILON)) saturated to int16 inside the ROI, the
//                       input disparity outside (W6)
// The two planes share a, b, c and t of a line: one lane computes them once and sweeps both.
#include "svo_internal.h"
#include "bm_plan.hip.h"

#include <cfloat>
#include <cmath>

namespace {

constexpr int WLS_ROWS = 64;   // rows per workgroup of the horizontal sweep (one wave, one lane per row)
constexpr int WLS_HT = 32;     // columns per LDS tile
constexpr int WLS_MAX_RADIUS = 255;
constexpr int WLS_NUM_ITER = 3;

struct WlsGeom {
    int w, h, c;
    int x0, y0, rw, rh;   // the left view's ROI
    int xr0;              // first column of the right view's ROI
    size_t img;           // w * h
    size_t roi;           // rw * rh
};

// cv::borderInterpolate(p, n, BORDER_REFLECT_101)
__device__ __forceinline__ int reflect101(int p, int n)
{
    if (n == 1)
        return 0;
    while (p < 0 || p >= n) {
        if (p < 0)
            p = -p;
        else
            p = 2 * (n - 1) - p;
    }
    return p;
}

// ---- W3: the box sums of one view's ROI crop ------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void wls_box_h_kernel(WlsGeom g, const int16_t *__restrict__ disp, int xv0, int radius,
                                                        long long *__restrict__ s2, int *__restrict__ s1)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= g.roi)
        return;
    const int pair = blockIdx.y, x = (int)(i % g.rw), y = (int)(i / g.rw);
    const int16_t *__restrict__ row = disp + pair * g.img + (size_t)(g.y0 + y) * g.w + xv0;
    int a = 0;
    long long b = 0;
    for (int k = -radius; k <= radius; k++) {
        const int v = row[reflect101(x + k, g.rw)];
        a += v;
        b += v * v;
    }
    s1[pair * g.roi + i] = a;
    s2[pair * g.roi + i] = b;
}

__global__ __launch_bounds__(256) void wls_box_v_kernel(WlsGeom g, const long long *__restrict__ s2, const int *__restrict__ s1,
                                                        int radius, float roll_off, double scale, float *__restrict__ dd)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= g.roi)
        return;
    const int pair = blockIdx.y, x = (int)(i % g.rw), y = (int)(i / g.rw);
    const size_t base = pair * g.roi + x;
    long long a = 0, b = 0;
    for (int k = -radius; k <= radius; k++) {
        const size_t o = base + (size_t)reflect101(y + k, g.rh) * g.rw;
        a += s1[o];
        b += s2[o];
    }
    const float mean = (float)((double)a * scale), meansq = (float)((double)b * scale);
    const float var = meansq - mean * mean;
    dd[pair * g.roi + i] = fmaxf(0.f, 1.f - roll_off * var);
}

// ---- W4 + the planes the smoother starts from --------------------------------------------------------------------------
__global__ __launch_bounds__(256) void wls_conf_kernel(WlsGeom g, const int16_t *__restrict__ dl, const int16_t *__restrict__ dr,
                                                       const float *__restrict__ ddl, const float *__restrict__ ddr, int thresh,
                                                       int use_conf, float *__restrict__ num, float *__restrict__ den,
                                                       float *__restrict__ conf_out)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= g.img)
        return;
    const int pair = blockIdx.y, x = (int)(i % g.w), y = (int)(i / g.w);
    const int rx = x - g.x0, ry = y - g.y0;
    float conf = 0.f;
    if (rx >= 0 && rx < g.rw && ry >= 0 && ry < g.rh) {
        const size_t o = pair * g.roi + (size_t)ry * g.rw + rx;
        const int d = dl[pair * g.img + i];
        if (use_conf) {
            const int xr = x - (d >> 4);
            if (xr >= g.xr0 && xr < g.xr0 + g.rw) {
                const int e = dr[pair * g.img + (size_t)y * g.w + xr];
                if (abs(d + e) < thresh)
                    conf = fminf(ddl[o], ddr[pair * g.roi + (size_t)ry * g.rw + (xr - g.xr0)]);
            }
            num[o] = (float)d * conf;
            den[o] = conf;
        } else {
            num[o] = (float)d;
        }
    }
    if (conf_out)
        conf_out[pair * g.img + i] = conf * 255.f;
}

// ---- W5: the weights -------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int guide_diff(const uint8_t *__restrict__ p, const uint8_t *__restrict__ q, int c)
{
    if (c == 1)
        return abs((int)p[0] - (int)q[0]);
    const int b = (int)p[0] - (int)q[0], gg = (int)p[1] - (int)q[1], r = (int)p[2] - (int)q[2];
    return b * b + gg * gg + r * r;
}

__global__ __launch_bounds__(256) void wls_weights_kernel(WlsGeom g, const uint8_t *__restrict__ guide, const float *__restrict__ lut,
                                                          float *__restrict__ chor, float *__restrict__ cvert)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= g.roi)
        return;
    const int pair = blockIdx.y, x = (int)(i % g.rw), y = (int)(i / g.rw);
    const uint8_t *__restrict__ p = guide + (pair * g.img + (size_t)(g.y0 + y) * g.w + g.x0 + x) * g.c;
    chor[pair * g.roi + i] = x + 1 < g.rw ? lut[guide_diff(p, p + g.c, g.c)] : 0.f;
    cvert[pair * g.roi + i] = y + 1 < g.rh ? lut[guide_diff(p, p + (size_t)g.w * g.c, g.c)] : 0.f;
}

// ---- W5: one step of the forward elimination; cp / tp / up: C, t and u of the previous element (0 before the first) ---------
template <int NP>
__device__ __forceinline__ void fgs_forward(float lam, float cj, float &cp, float &tp, float (&u)[NP], float (&up)[NP], float &t)
{
    const float a = lam * cp, c = lam * cj;
    const float b = (1.f - a) - c;
    const float den = b - a * tp;   // j = 0: a = 0, tp = 0 -> b itself
    t = c / den;
#pragma unroll
    for (int p = 0; p < NP; p++) {
        u[p] = (u[p] - a * up[p]) / den;
        up[p] = u[p];
    }
    cp = cj;
    tp = t;
}

// ---- the horizontal sweep: 64 rows per wave, tiles transposed through LDS ---------------------------------------------------
template <int NP>
__global__ __launch_bounds__(WLS_ROWS) void wls_hsweep_kernel(WlsGeom g, float lam, const float *__restrict__ C, float *__restrict__ T,
                                                              float *__restrict__ P0, float *__restrict__ P1)
{
    __shared__ float sc[WLS_ROWS][WLS_HT + 1], st[WLS_ROWS][WLS_HT + 1], su[NP][WLS_ROWS][WLS_HT + 1];
    const int lane = threadIdx.x, row0 = blockIdx.x * WLS_ROWS, pair = blockIdx.y, rw = g.rw;
    const int nrows = min(WLS_ROWS, g.rh - row0);
    const size_t base = pair * g.roi + (size_t)row0 * rw;
    float *__restrict__ P[2] = {P0, P1};
    const int ntiles = (rw + WLS_HT - 1) / WLS_HT;
    float cp = 0.f, tp = 0.f, up[NP], u[NP];
#pragma unroll
    for (int p = 0; p < NP; p++)
        up[p] = 0.f;
    for (int tile = 0; tile < ntiles; tile++) {
        const int x0 = tile * WLS_HT, nx = min(WLS_HT, rw - x0);
        for (int e = lane; e < WLS_ROWS * WLS_HT; e += WLS_ROWS) {
            const int r = e / WLS_HT, cx = e % WLS_HT;
            if (r < nrows && cx < nx) {
                const size_t o = base + (size_t)r * rw + x0 + cx;
                sc[r][cx] = C[o];
#pragma unroll
                for (int p = 0; p < NP; p++)
                    su[p][r][cx] = P[p][o];
            }
        }
        __syncthreads();
        if (lane < nrows)
            for (int cx = 0; cx < nx; cx++) {
                float t;
#pragma unroll
                for (int p = 0; p < NP; p++)
                    u[p] = su[p][lane][cx];
                fgs_forward<NP>(lam, sc[lane][cx], cp, tp, u, up, t);
                st[lane][cx] = t;
#pragma unroll
                for (int p = 0; p < NP; p++)
                    su[p][lane][cx] = u[p];
            }
        __syncthreads();
        for (int e = lane; e < WLS_ROWS * WLS_HT; e += WLS_ROWS) {
            const int r = e / WLS_HT, cx = e % WLS_HT;
            if (r < nrows && cx < nx) {
                const size_t o = base + (size_t)r * rw + x0 + cx;
                T[o] = st[r][cx];
#pragma unroll
                for (int p = 0; p < NP; p++)
                    P[p][o] = su[p][r][cx];
            }
        }
        __syncthreads();
    }
    // back substitution, right to left; up: u of the element to the right
    for (int tile = ntiles - 1; tile >= 0; tile--) {
        const int x0 = tile * WLS_HT, nx = min(WLS_HT, rw - x0);
        for (int e = lane; e < WLS_ROWS * WLS_HT; e += WLS_ROWS) {
            const int r = e / WLS_HT, cx = e % WLS_HT;
            if (r < nrows && cx < nx) {
                const size_t o = base + (size_t)r * rw + x0 + cx;
                st[r][cx] = T[o];
#pragma unroll
                for (int p = 0; p < NP; p++)
                    su[p][r][cx] = P[p][o];
            }
        }
        __syncthreads();
        if (lane < nrows)
            for (int cx = nx - 1; cx >= 0; cx--) {
                const float t = st[lane][cx];
                const bool last = x0 + cx == rw - 1;
#pragma unroll
                for (int p = 0; p < NP; p++) {
                    const float v = su[p][lane][cx];
                    up[p] = last ? v : v - t * up[p];
                    su[p][lane][cx] = up[p];
                }
            }
        __syncthreads();
        for (int e = lane; e < WLS_ROWS * WLS_HT; e += WLS_ROWS) {
            const int r = e / WLS_HT, cx = e % WLS_HT;
            if (r < nrows && cx < nx) {
                const size_t o = base + (size_t)r * rw + x0 + cx;
#pragma unroll
                for (int p = 0; p < NP; p++)
                    P[p][o] = su[p][r][cx];
            }
        }
        __syncthreads();
    }
}

// ---- the vertical sweep: one lane per column ---------------------------------------------------------------------------------
template <int NP>
__global__ __launch_bounds__(64) void wls_vsweep_kernel(WlsGeom g, float lam, const float *__restrict__ C, float *__restrict__ T,
                                                        float *__restrict__ P0, float *__restrict__ P1)
{
    const int x = blockIdx.x * 64 + threadIdx.x, pair = blockIdx.y, rw = g.rw, rh = g.rh;
    if (x >= rw)
        return;
    const size_t base = pair * g.roi + x;
    float *__restrict__ P[2] = {P0, P1};
    float cp = 0.f, tp = 0.f, up[NP], u[NP];
#pragma unroll
    for (int p = 0; p < NP; p++)
        up[p] = 0.f;
    for (int y = 0; y < rh; y++) {
        const size_t o = base + (size_t)y * rw;
        float t;
#pragma unroll
        for (int p = 0; p < NP; p++)
            u[p] = P[p][o];
        fgs_forward<NP>(lam, C[o], cp, tp, u, up, t);
        T[o] = t;
#pragma unroll
        for (int p = 0; p < NP; p++)
            P[p][o] = u[p];
    }
    for (int y = rh - 2; y >= 0; y--) {
        const size_t o = base + (size_t)y * rw;
        const float t = T[o];
#pragma unroll
        for (int p = 0; p < NP; p++) {
            up[p] = P[p][o] - t * up[p];
            P[p][o] = up[p];
        }
    }
}

// ---- W6 -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void wls_finish_kernel(WlsGeom g, const int16_t *__restrict__ dl, const float *__restrict__ num,
                                                         const float *__restrict__ den, int use_conf, int16_t *__restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= g.img)
        return;
    const int pair = blockIdx.y, x = (int)(i % g.w), y = (int)(i / g.w);
    const int rx = x - g.x0, ry = y - g.y0;
    int v = dl[pair * g.img + i];
    if (rx >= 0 && rx < g.rw && ry >= 0 && ry < g.rh) {
        const size_t o = pair * g.roi + (size_t)ry * g.rw + rx;
        float q = num[o];
        if (use_conf)
            q = q / (den[o] + FLT_EPSILON);
        q = rintf(q);   // half to even
        v = q >= 32767.f ? 32767 : (q <= -32768.f ? -32768 : (int)q);
    }
    out[pair * g.img + i] = (int16_t)v;
}

__global__ __launch_bounds__(256) void wls_grey_kernel(const uint8_t *__restrict__ bgr, uint8_t *__restrict__ grey, size_t n)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n)
        grey[i] = (uint8_t)svo_bgr2gray(bgr[3 * i], bgr[3 * i + 1], bgr[3 * i + 2]);
}

int wls_check(const svo_wls_params *p, int w, int h, int c, int n_pairs, WlsGeom *g)
{
    SVO_CHECK_ARG(p != nullptr);
    SVO_CHECK_ARG(n_pairs >= 1 && n_pairs <= SVO_LK_MAX_JOBS);
    SVO_CHECK_ARG(c == 1 || c == 3);
    SVO_CHECK_ARG(w >= 1 && h >= 1);
    SVO_CHECK_ARG(p->lambda >= 0 && p->sigma_color > 0);   // NaN fails both
    SVO_CHECK_ARG(p->depth_discontinuity_radius >= 0);
    SVO_CHECK_ARG(p->roi_left >= 0 && p->roi_right >= 0 && p->roi_top >= 0 && p->roi_bottom >= 0);
    SVO_CHECK_ARG((long long)p->roi_left + p->roi_right < w && (long long)p->roi_top + p->roi_bottom < h);   // an empty ROI
    if (p->depth_discontinuity_radius > WLS_MAX_RADIUS) {
        svo_set_error("svo_wls_filter: depth_discontinuity_radius above %d", WLS_MAX_RADIUS);
        return SVO_ERR_CAPACITY;
    }
    if ((long long)w * h * n_pairs >= (1LL << 30)) {
        svo_set_error("svo_wls_filter: 2^30 pixels or more per call");
        return SVO_ERR_CAPACITY;
    }
    g->w = w, g->h = h, g->c = c;
    g->x0 = p->roi_left, g->y0 = p->roi_top;
    g->rw = w - p->roi_left - p->roi_right, g->rh = h - p->roi_top - p->roi_bottom;
    g->xr0 = w - (g->x0 + g->rw);
    g->img = (size_t)w * h;
    g->roi = (size_t)g->rw * g->rh;
    return SVO_OK;
}

// W5: the table on the device, kept in the context until sigma or the channel count changes
int wls_table(svo_ctx *ctx, double sigma, int c, const float **out)
{
    const int n = c == 1 ? 256 : 3 * 255 * 255 + 1;
    if (!(ctx->wls_lut.p && ctx->wls_lut_c == c && ctx->wls_lut_sigma == sigma)) {
        int rc;
        if ((rc = ctx->wls_lut.ensure((size_t)n * sizeof(float))))
            return rc;
        ctx->wls_lut_c = 0;
        ctx->wls_lut_host.resize((size_t)n);
        for (int k = 0; k < n; k++) {
            const double d = c == 1 ? (double)k : std::sqrt((double)k);
            ctx->wls_lut_host[(size_t)k] = (float)(-svo_exp(-d / sigma));
        }
        // the stream may still be reading the table of an earlier call
        SVO_HIP(hipStreamSynchronize(ctx->stream));
        SVO_HIP(hipMemcpyAsync(ctx->wls_lut.p, ctx->wls_lut_host.data(), (size_t)n * sizeof(float), hipMemcpyHostToDevice,
                               ctx->stream));
        SVO_HIP(hipStreamSynchronize(ctx->stream));
        ctx->wls_lut_c = c;
        ctx->wls_lut_sigma = sigma;
    }
    *out = ctx->wls_lut.as<float>();
    return SVO_OK;
}

template <int NP>
void wls_sweeps(hipStream_t st, const WlsGeom &g, int n, float lam, const float *chor, const float *cvert, float *T, float *num,
                float *den)
{
    const dim3 gh((unsigned)((g.rh + WLS_ROWS - 1) / WLS_ROWS), n), gv((unsigned)((g.rw + 63) / 64), n);
    for (int it = 0; it < WLS_NUM_ITER; it++) {
        hipLaunchKernelGGL(wls_hsweep_kernel<NP>, gh, dim3(WLS_ROWS), 0, st, g, lam, chor, T, num, den);
        hipLaunchKernelGGL(wls_vsweep_kernel<NP>, gv, dim3(64), 0, st, g, lam, cvert, T, num, den);
        lam = lam * 0.25f;
    }
}

// everything on the device: dl / dr n x h x w int16, guide n x h x w x c, out n x h x w int16, conf_out n x h x w float or null
int wls_run(svo_ctx *ctx, const svo_wls_params *p, const WlsGeom &g, int n, const int16_t *dl, const int16_t *dr,
            const uint8_t *guide, int16_t *out, float *conf_out)
{
    hipStream_t st = ctx->stream;
    const float *lut = nullptr;
    int rc;
    if ((rc = wls_table(ctx, p->sigma_color, g.c, &lut)))
        return rc;
    // seven float planes per ROI pixel: dd_l, dd_r, num, den, Chor, Cvert, t.  The box sums (8 + 4 bytes per pixel) are
    // gone before the weights are written and lie over Chor / Cvert / t.
    const size_t M = (((size_t)n * g.roi + 63) / 64) * 64;
    if ((rc = ctx->wls_work.ensure(M * 7 * sizeof(float) + 256)))
        return rc;
    float *ddl = ctx->wls_work.as<float>(), *ddr = ddl + M, *num = ddr + M, *den = num + M, *chor = den + M, *cvert = chor + M,
          *T = cvert + M;
    long long *s2 = reinterpret_cast<long long *>(chor);
    int *s1 = reinterpret_cast<int *>(chor + 2 * M);
    const int use_conf = p->use_confidence ? 1 : 0;
    const dim3 groi((unsigned)((g.roi + 255) / 256), n), gimg((unsigned)((g.img + 255) / 256), n);
    if (use_conf) {
        const int r = p->depth_discontinuity_radius;
        const double scale = 1.0 / (double)((2 * r + 1) * (2 * r + 1));
        hipLaunchKernelGGL(wls_box_h_kernel, groi, dim3(256), 0, st, g, dl, g.x0, r, s2, s1);
        hipLaunchKernelGGL(wls_box_v_kernel, groi, dim3(256), 0, st, g, s2, s1, r, p->roll_off, scale, ddl);
        hipLaunchKernelGGL(wls_box_h_kernel, groi, dim3(256), 0, st, g, dr, g.xr0, r, s2, s1);
        hipLaunchKernelGGL(wls_box_v_kernel, groi, dim3(256), 0, st, g, s2, s1, r, p->roll_off, scale, ddr);
    }
    hipLaunchKernelGGL(wls_conf_kernel, gimg, dim3(256), 0, st, g, dl, dr, ddl, ddr, p->lrc_thresh, use_conf, num, den, conf_out);
    hipLaunchKernelGGL(wls_weights_kernel, groi, dim3(256), 0, st, g, guide, lut, chor, cvert);
    const float lam = (float)(1.5 * p->lambda * 16.0 / 63.0);   // 4^(n-1) / (4^n - 1), n = 3
    if (use_conf)
        wls_sweeps<2>(st, g, n, lam, chor, cvert, T, num, den);
    else
        wls_sweeps<1>(st, g, n, lam, chor, cvert, T, num, den);
    hipLaunchKernelGGL(wls_finish_kernel, gimg, dim3(256), 0, st, g, dl, num, den, use_conf, out);
    SVO_HIP(hipGetLastError());
    return SVO_OK;
}

// The chain of svo_sgbm_wls_compute and svo_bm_wls_compute: the left matcher, the right matcher `rp` on the swapped images (only
// when the filter or the caller wants its map), the grey guide, the filter.  compute: svo_sgbm_compute or svo_bm_compute.
template <class Params, class Compute>
int wls_matcher_chain(svo_ctx *ctx, const Params *sp, const Params &rp_in, Compute compute, const svo_wls_params *wp, const WlsGeom &g,
                      bool want_right, const uint8_t *left, const uint8_t *right, int w, int h, int c, int n_pairs,
                      int16_t *filtered, int16_t *disp_left, int16_t *disp_right, float *confidence, int mem)
{
    const Params rp = rp_in;
    int rc;
    SVO_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t npix = (size_t)n_pairs * g.img, img_bytes = npix * c;
    const uint8_t *dleft = left, *dright = right;
    const bool host = mem == SVO_MEM_HOST;
    // the matchers' maps and the grey guide stay on the device between the passes: [left map | right map | filtered |
    // confidence | grey]
    const size_t plane = ((npix * 2 + 255) / 256) * 256;
    if ((rc = ctx->wls_maps.ensure(plane * 3 + npix * 4 + 256 + npix)))
        return rc;
    uint8_t *mb = ctx->wls_maps.as<uint8_t>();
    int16_t *m_l = reinterpret_cast<int16_t *>(mb), *m_r = reinterpret_cast<int16_t *>(mb + plane),
            *m_f = reinterpret_cast<int16_t *>(mb + 2 * plane);
    float *m_c = reinterpret_cast<float *>(mb + 3 * plane);
    uint8_t *m_g = mb + 3 * plane + ((npix * 4 + 255) / 256) * 256;
    if (host) {
        if ((rc = ctx->s_a.ensure(img_bytes)) || (rc = ctx->s_b.ensure(img_bytes)))
            return rc;
        SVO_HIP(hipMemcpyAsync(ctx->s_a.p, left, img_bytes, hipMemcpyHostToDevice, st));
        SVO_HIP(hipMemcpyAsync(ctx->s_b.p, right, img_bytes, hipMemcpyHostToDevice, st));
        dleft = ctx->s_a.as<uint8_t>();
        dright = ctx->s_b.as<uint8_t>();
    }
    // every output is written at the end, from the maps kept here: a refusal on the way leaves them untouched
    if ((rc = compute(ctx, sp, dleft, dright, w, h, c, n_pairs, m_l, SVO_MEM_DEVICE)))
        return rc;
    if (want_right && (rc = compute(ctx, &rp, dright, dleft, w, h, c, n_pairs, m_r, SVO_MEM_DEVICE)))
        return rc;
    const uint8_t *guide = dleft;
    if (c == 3) {
        hipLaunchKernelGGL(wls_grey_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, st, dleft, m_g, npix);
        guide = m_g;
    }
    if ((rc = wls_run(ctx, wp, g, n_pairs, m_l, m_r, guide, m_f, confidence ? m_c : nullptr)))
        return rc;
    const hipMemcpyKind kind = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    SVO_HIP(hipMemcpyAsync(filtered, m_f, npix * 2, kind, st));
    if (disp_left)
        SVO_HIP(hipMemcpyAsync(disp_left, m_l, npix * 2, kind, st));
    if (disp_right)
        SVO_HIP(hipMemcpyAsync(disp_right, m_r, npix * 2, kind, st));
    if (confidence)
        SVO_HIP(hipMemcpyAsync(confidence, m_c, npix * 4, kind, st));
    if (host)
        SVO_HIP(hipStreamSynchronize(st));
    return SVO_OK;
}

}  // namespace

extern "C" {

void svo_sgbm_right_matcher_params(const svo_sgbm_params *left, svo_sgbm_params *right)
{
    if (!left || !right)
        return;
    const svo_sgbm_params l = *left;
    *right = l;
    right->min_disparity = -(l.min_disparity + l.num_disparities) + 1;
    right->uniqueness_ratio = 0;
    right->disp12_max_diff = 1000000;
    right->speckle_window_size = 0;
    right->speckle_range = 0;
}

void svo_wls_default_params(const svo_sgbm_params *left, svo_wls_params *out)
{
    if (!left || !out)
        return;
    const int block = left->block_size, half = block / 2, maxd = left->min_disparity + left->num_disparities;
    out->lambda = 8000.0;
    out->sigma_color = 1.5;
    out->lrc_thresh = 24;
    out->depth_discontinuity_radius = block > 0 ? (block + 1) / 2 : 0;   // ceil(0.5 * block)
    out->roll_off = 0.001f;
    out->use_confidence = 1;
    out->roi_left = (maxd > 0 ? maxd : 0) + half;
    out->roi_right = (left->min_disparity < 0 ? -left->min_disparity : 0) + half;
    out->roi_top = out->roi_bottom = half;
}

int svo_wls_filter(svo_ctx *ctx, const svo_wls_params *p, const int16_t *disp_left, const int16_t *disp_right, const uint8_t *guide,
                   int w, int h, int c, int n_pairs, int16_t *filtered, float *confidence, int mem)
{
    WlsGeom g;
    int rc;
    if ((rc = wls_check(p, w, h, c, n_pairs, &g)))
        return rc;
    SVO_CHECK_ARG(ctx && disp_left && guide && filtered);
    SVO_CHECK_ARG(disp_right || !p->use_confidence);
    SVO_CHECK_ARG(mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE);
    SVO_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t npix = (size_t)n_pairs * g.img;
    if (mem == SVO_MEM_DEVICE)
        return wls_run(ctx, p, g, n_pairs, disp_left, disp_right, guide, filtered, confidence);
    if ((rc = ctx->s_a.ensure(npix * 2)) || (rc = ctx->s_b.ensure(npix * 2)) || (rc = ctx->s_c.ensure(npix * c)) ||
        (rc = ctx->s_d.ensure(npix * 2)) || (rc = ctx->s_e.ensure(npix * 4)))
        return rc;
    SVO_HIP(hipMemcpyAsync(ctx->s_a.p, disp_left, npix * 2, hipMemcpyHostToDevice, st));
    if (p->use_confidence)
        SVO_HIP(hipMemcpyAsync(ctx->s_b.p, disp_right, npix * 2, hipMemcpyHostToDevice, st));
    SVO_HIP(hipMemcpyAsync(ctx->s_c.p, guide, npix * c, hipMemcpyHostToDevice, st));
    if ((rc = wls_run(ctx, p, g, n_pairs, ctx->s_a.as<int16_t>(), ctx->s_b.as<int16_t>(), ctx->s_c.as<uint8_t>(),
                      ctx->s_d.as<int16_t>(), confidence ? ctx->s_e.as<float>() : nullptr)))
        return rc;
    SVO_HIP(hipMemcpyAsync(filtered, ctx->s_d.p, npix * 2, hipMemcpyDeviceToHost, st));
    if (confidence)
        SVO_HIP(hipMemcpyAsync(confidence, ctx->s_e.p, npix * 4, hipMemcpyDeviceToHost, st));
    SVO_HIP(hipStreamSynchronize(st));
    return SVO_OK;
}

int svo_sgbm_wls_compute(svo_ctx *ctx, const svo_sgbm_params *sp, const svo_wls_params *wp, const uint8_t *left, const uint8_t *right,
                         int w, int h, int c, int n_pairs, int16_t *filtered, int16_t *disp_left, int16_t *disp_right,
                         float *confidence, int mem)
{
    WlsGeom g;
    int rc;
    SVO_CHECK_ARG(sp != nullptr);
    if ((rc = wls_check(wp, w, h, 1, n_pairs, &g)))   // the guide is the grey left image
        return rc;
    SVO_CHECK_ARG(ctx && left && right && filtered);
    SVO_CHECK_ARG(c == 1 || c == 3);
    SVO_CHECK_ARG(mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE);
    svo_sgbm_params rp;
    svo_sgbm_right_matcher_params(sp, &rp);
    const bool want_right = wp->use_confidence || disp_right;
    SVO_CHECK_ARG(!want_right || w > rp.num_disparities + rp.min_disparity);   // what the right matcher would refuse
    return wls_matcher_chain(ctx, sp, rp, svo_sgbm_compute, wp, g, want_right, left, right, w, h, c, n_pairs, filtered, disp_left,
                             disp_right, confidence, mem);
}

void svo_bm_right_matcher_params(const svo_bm_params *left, svo_bm_params *right)
{
    if (!left || !right)
        return;
    const svo_bm_params l = *left;
    *right = l;
    right->min_disparity = -(l.min_disparity + l.num_disparities) + 1;
    right->texture_threshold = 0;
    right->uniqueness_ratio = 0;
    right->disp12_max_diff = 1000000;
    right->speckle_window_size = 0;
    right->speckle_range = 0;
}

void svo_wls_default_params_bm(const svo_bm_params *left, svo_wls_params *out)
{
    if (!left || !out)
        return;
    svo_sgbm_params range;   // the ROI and the other values are the SGBM case's, formed from the range and the block alone
    svo_sgbm_default_params(&range);
    range.min_disparity = left->min_disparity;
    range.num_disparities = left->num_disparities;
    range.block_size = left->block_size;
    svo_wls_default_params(&range, out);
    out->depth_discontinuity_radius = left->block_size > 0 ? (int)((33ll * left->block_size + 99) / 100) : 0;   // ceil(0.33 * block)
}

int svo_bm_wls_compute(svo_ctx *ctx, const svo_bm_params *bp, const svo_wls_params *wp, const uint8_t *left, const uint8_t *right,
                       int w, int h, int c, int n_pairs, int16_t *filtered, int16_t *disp_left, int16_t *disp_right,
                       float *confidence, int mem)
{
    WlsGeom g;
    int rc;
    SVO_CHECK_ARG(bp != nullptr);
    if ((rc = wls_check(wp, w, h, 1, n_pairs, &g)))   // the guide is the grey left image
        return rc;
    const char *why = nullptr;
    if ((rc = bm_plan::check(bp, w, h, c, n_pairs, &why))) {   // the matcher's refusals, before anything is touched
        svo_set_error("svo_bm_wls_compute: %s", why);
        return rc == 1 ? SVO_ERR_ARG : SVO_ERR_CAPACITY;
    }
    SVO_CHECK_ARG(ctx && left && right && filtered);
    SVO_CHECK_ARG(mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE);
    // the right matcher refuses what the left one does (the same sizes and block; an empty band is no refusal), and the left
    // one runs first, into the chain's own maps
    svo_bm_params rp;
    svo_bm_right_matcher_params(bp, &rp);
    return wls_matcher_chain(ctx, bp, rp, svo_bm_compute, wp, g, wp->use_confidence || disp_right, left, right, w, h, c, n_pairs,
                             filtered, disp_left, disp_right, confidence, mem);
}

}  // extern "C"
