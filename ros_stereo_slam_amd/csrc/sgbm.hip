// sgbm.hip -- dense stereo: cv::StereoSGBM (MODE_SGBM) as StereoProcess::stereoMatch calls it (src/StereoCV.cpp:21-59),
// and reprojectImageTo3D + the window / flip / colour loop of StereoProcess::reprojectDisparity (src/StereoCV.cpp:227-250).
// The recipe and every recalled point of it: tests/sgbm_numpy.py (R1..R16), DESIGN.md section 10.  Integer arithmetic
// throughout; the results are bit-identical to the restatement.
//
// Per call (n pairs, blockIdx.y / .z = pair):
//   sgbm_hsum_kernel    one workgroup per row: grey (cv_gray weights), pre-filter, Birchfield-Tomasi pixel costs of a
//                       tile of band columns into LDS, the horizontal block sum -> hsum [pair][y][x][d] (int16, d fastest)
//   sgbm_vsum_kernel    one thread per (x, d): the vertical block sum down the column with 3.2's quirks (R5) -> C
//   sgbm_path_kernel    one wave per path line of the four top-to-bottom directions; a lane owns PER consecutive
//                       disparities, Lr'(d +- 1) across lanes by shuffles, minLr' by a butterfly min; Lr of the previous
//                       step in registers; each direction writes its own plane (the sum of the four is formed once,
//                       in int, by the WTA kernel: S = sat16(L0 + L1 + L2 + L3) exactly as the sequential sweep).
//                       The planes are int16 while every L provably fits (see planes_need_int); beyond that C and the
//                       stored Lr wrap, the sweep still sums the int L (R7), and the planes are kept as int
//   sgbm_wta_kernel     one wave per row: the right->left path, S, winner-take-all, uniqueness, sub-pixel, disp2 in LDS
//                       (serial in x, so the tie rule is the reference's), then the left-right check over the row
//   sgbm_median_kernel  medianBlur 3x3, replicated border (R12)
//   speckle_*_kernel    filterSpeckles as union-find: link by atomicMin on roots, compress, count by atomicAdd (one per
//                       distinct root of a wave),
//                       invalidate components of <= window pixels (the partition is unique: the result does not depend
//                       on the order threads run in)
#include "svo_internal.h"
#include "wave_ops.hip.h"

#include <climits>

namespace {

constexpr int SGBM_MAXW = 2048;      // widest image (LDS rows of the cost kernel: 57 KB per workgroup)
constexpr int SGBM_TX = 32;          // band columns per pixel-cost tile
constexpr size_t SGBM_MAX_CELLS = (size_t)1 << 30;   // cost cells (pairs x rows x band columns x D) per call
constexpr int SHORT_MAX_ = 32767;

struct SgbmGeom {
    int w, h, c, minD, D, minX1, width1, P1, P2, ftzero, ratio, maxdiff, SW2, SH2;
    size_t img_stride;   // bytes per input image
    size_t cells;        // h * width1 * D: cells of one pair's plane
    size_t plane_stride; // cells of one direction's plane over all pairs of the call
};

__device__ __forceinline__ int sat16(int v) { return v < -32768 ? -32768 : (v > SHORT_MAX_ ? SHORT_MAX_ : v); }

__device__ __forceinline__ int grey_at(const uint8_t *__restrict__ img, int c, size_t i)
{
    if (c == 1)
        return img[i];
    const uint8_t *p = img + 3 * i;
    return (1868 * p[0] + 9617 * p[1] + 4899 * p[2] + 8192) >> 14;
}

// ---- pixel costs + horizontal block sum ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sgbm_hsum_kernel(SgbmGeom g, const uint8_t *__restrict__ left,
                                                        const uint8_t *__restrict__ right, int16_t *__restrict__ hsum)
{
    __shared__ uint8_t grey[2][3][SGBM_MAXW];
    // [image][channel][x]: value, half-sample min, half-sample max (R3)
    __shared__ uint8_t val[2][2][SGBM_MAXW], vmin[2][2][SGBM_MAXW], vmax[2][2][SGBM_MAXW];
    __shared__ int16_t pix[(SGBM_TX + 10) * 256];
    const int y = blockIdx.x, pair = blockIdx.y, t = threadIdx.x, w = g.w;
    const uint8_t *imgs[2] = {left + pair * g.img_stride, right + pair * g.img_stride};
    const int rows[3] = {y > 0 ? y - 1 : y, y, y < g.h - 1 ? y + 1 : y};
    for (int i = 0; i < 2; i++)
        for (int r = 0; r < 3; r++)
            for (int x = t; x < w; x += 256)
                grey[i][r][x] = (uint8_t)grey_at(imgs[i], g.c, (size_t)rows[r] * w + x);
    __syncthreads();
    for (int i = 0; i < 2; i++)
        for (int x = t; x < w; x += 256) {
            int der = g.ftzero, inten = g.ftzero;   // columns 0 and w-1 of both channels: tab[0] (R2)
            if (x >= 1 && x < w - 1) {
                const int v = (grey[i][1][x + 1] - grey[i][1][x - 1]) * 2 + grey[i][0][x + 1] - grey[i][0][x - 1] +
                              grey[i][2][x + 1] - grey[i][2][x - 1];
                der = min(max(v, -g.ftzero), g.ftzero) + g.ftzero;
                inten = grey[i][1][x];
            }
            val[i][0][x] = (uint8_t)der;
            val[i][1][x] = (uint8_t)inten;
        }
    __syncthreads();
    for (int i = 0; i < 2; i++)
        for (int ch = 0; ch < 2; ch++)
            for (int x = t; x < w; x += 256) {
                const int v = val[i][ch][x];
                const int vl = x > 0 ? (v + val[i][ch][x - 1]) / 2 : v;
                const int vr = x < w - 1 ? (v + val[i][ch][x + 1]) / 2 : v;
                vmin[i][ch][x] = (uint8_t)min(min(vl, vr), v);
                vmax[i][ch][x] = (uint8_t)max(max(vl, vr), v);
            }
    __syncthreads();
    const int D = g.D, SW2 = g.SW2, width1 = g.width1, span = SGBM_TX + 2 * SW2;
    int16_t *__restrict__ out = hsum + pair * g.cells + (size_t)y * width1 * D;
    for (int x0 = 0; x0 < width1; x0 += SGBM_TX) {
        // pixel costs of band columns clamp(x0 - SW2 .. x0 + TX + SW2 - 1) (R4: the band's edges replicate)
        for (int e = t; e < span * D; e += 256) {
            const int j = e / D, d = e - j * D;
            const int xb = min(max(x0 - SW2 + j, 0), width1 - 1);
            const int xl = g.minX1 + xb, xr = xl - (g.minD + d);
            int cost = 0;
#pragma unroll
            for (int ch = 0; ch < 2; ch++) {
                const int u = val[0][ch][xl], u0 = vmin[0][ch][xl], u1 = vmax[0][ch][xl];
                const int v = val[1][ch][xr], v0 = vmin[1][ch][xr], v1 = vmax[1][ch][xr];
                const int c0 = max(max(0, u - v1), v0 - u);
                const int c1 = max(max(0, v - u1), u0 - v);
                cost += min(c0, c1) >> (ch ? 2 : 0);
            }
            pix[e] = (int16_t)cost;
        }
        __syncthreads();
        const int nx = min(SGBM_TX, width1 - x0);
        for (int e = t; e < nx * D; e += 256) {
            const int j = e / D, d = e - j * D;
            int s = 0;
            for (int k = 0; k <= 2 * SW2; k++)
                s += pix[(j + k) * D + d];
            out[(size_t)(x0 + j) * D + d] = (int16_t)s;
        }
        __syncthreads();
    }
}

// ---- vertical block sum (R5) ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sgbm_vsum_kernel(SgbmGeom g, const int16_t *__restrict__ hsum, int16_t *__restrict__ C)
{
    const int col = blockIdx.x * 256 + threadIdx.x, pair = blockIdx.y;
    const int D = g.D, h = g.h, SH2 = g.SH2;
    const size_t row = (size_t)g.width1 * D;
    if (col >= (int)row)
        return;
    const int16_t *__restrict__ hs = hsum + pair * g.cells + col;
    int16_t *__restrict__ out = C + pair * g.cells + col;
    int c = g.P2;
    for (int k = 0; k <= SH2; k++)
        c += hs[(size_t)min(k, h - 1) * row] * (k == 0 ? SH2 + 1 : 1);
    int16_t cur = (int16_t)c;
    out[0] = cur;
    const bool first_col = col < D;   // the band's first column keeps its row-0 value
    for (int y = 1; y < h; y++) {
        if (y + SH2 < h && !first_col)
            cur = (int16_t)(cur + hs[(size_t)(y + SH2) * row] - hs[(size_t)max(y - SH2 - 1, 0) * row]);
        out[(size_t)y * row] = cur;
    }
}

// one step of R6 for the PER disparities of this lane; Lp / minLp: the stored int16 values of the previous step
template <int PER>
__device__ __forceinline__ void path_step(const int (&Cv)[PER], int (&Lp)[PER], int &minLp, int (&L)[PER], bool last_lane,
                                          int P1, int P2)
{
    const int lane = threadIdx.x & 63;
    int lm = __shfl_up(Lp[PER - 1], 1);
    int rn = __shfl_down(Lp[0], 1);
    if (lane == 0)
        lm = SHORT_MAX_;
    if (last_lane)
        rn = SHORT_MAX_;
    const int delta = minLp + P2;
#pragma unroll
    for (int k = 0; k < PER; k++) {
        const int a = k ? Lp[k - 1] : lm, b = k < PER - 1 ? Lp[k + 1] : rn;
        L[k] = Cv[k] + min(min(Lp[k], a + P1), min(b + P1, delta)) - delta;
    }
}

template <int PER> __device__ __forceinline__ void load_c(const int16_t *p, bool active, int (&v)[PER])
{
#pragma unroll
    for (int k = 0; k < PER; k++)
        v[k] = active ? p[k] : 0;
}

// ---- the four top-to-bottom directions: one wave per line ---------------------------------------------------------------
template <int PER, class PlaneT>
__global__ __launch_bounds__(256) void sgbm_path_kernel(SgbmGeom g, const int16_t *__restrict__ C, PlaneT *__restrict__ planes,
                                                        int n_lines)
{
    const int wave = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, pair = blockIdx.y;
    if (wave >= n_lines)
        return;
    const int H = g.h, W1 = g.width1, D = g.D;
    int dir, x0, y0, dx, dy, len, li = wave;
    if (li < H) {                       // left -> right, one line per row
        dir = 0, x0 = 0, y0 = li, dx = 1, dy = 0, len = W1;
    } else if ((li -= H) < W1) {        // top -> bottom, one line per column
        dir = 2, x0 = li, y0 = 0, dx = 0, dy = 1, len = H;
    } else if ((li -= W1) < W1 + H - 1) {   // from (x-1, y-1): starts on the top row and on the left edge
        dir = 1, dx = 1, dy = 1;
        if (li < W1)
            x0 = li, y0 = 0;
        else
            x0 = 0, y0 = li - W1 + 1;
        len = min(W1 - x0, H - y0);
    } else {                            // from (x+1, y-1): starts on the top row and on the right edge
        li -= W1 + H - 1;
        dir = 3, dx = -1, dy = 1;
        if (li < W1)
            x0 = li, y0 = 0;
        else
            x0 = W1 - 1, y0 = li - W1 + 1;
        len = min(x0 + 1, H - y0);
    }
    const bool active = lane * PER < D, last_lane = (lane + 1) * PER >= D;
    const int16_t *__restrict__ Cp = C + pair * g.cells + lane * PER;
    PlaneT *__restrict__ plane = planes + (size_t)dir * g.plane_stride + pair * g.cells + lane * PER;
    int Lp[PER], L[PER], Cv[PER], Cn[PER];
#pragma unroll
    for (int k = 0; k < PER; k++)
        Lp[k] = 0;
    int minLp = 0;
    size_t off = ((size_t)y0 * W1 + x0) * D;
    const ptrdiff_t step = ((ptrdiff_t)dy * W1 + dx) * D;
    load_c<PER>(Cp + off, active, Cn);
    for (int s = 0; s < len; s++) {
#pragma unroll
        for (int k = 0; k < PER; k++)
            Cv[k] = Cn[k];
        if (s + 1 < len)
            load_c<PER>(Cp + off + step, active, Cn);
        path_step<PER>(Cv, Lp, minLp, L, last_lane, g.P1, g.P2);
        int mn = INT_MAX;
#pragma unroll
        for (int k = 0; k < PER; k++) {
            if (active)
                plane[off + k] = (PlaneT)L[k];
            mn = min(mn, L[k]);
            Lp[k] = (int16_t)L[k];
        }
        minLp = (int16_t)svo::wave_min(active ? mn : INT_MAX);
        off += step;
    }
}

// ---- right -> left path, S, winner-take-all, disp2, left-right check: one wave per row ---------------------------------
template <int PER, class PlaneT>
__global__ __launch_bounds__(64) void sgbm_wta_kernel(SgbmGeom g, const int16_t *__restrict__ C, const PlaneT *__restrict__ planes,
                                                      int16_t *__restrict__ raw)
{
    __shared__ int16_t drow[SGBM_MAXW], disp2[SGBM_MAXW];
    __shared__ int cost2[SGBM_MAXW];
    __shared__ int srow[256];
    const int y = blockIdx.x, pair = blockIdx.y, lane = threadIdx.x;
    const int w = g.w, W1 = g.width1, D = g.D, minD = g.minD, minX1 = g.minX1;
    const int invalid = (minD - 1) * 16;
    for (int x = lane; x < w; x += 64) {
        drow[x] = (int16_t)invalid;
        disp2[x] = (int16_t)invalid;
        cost2[x] = SHORT_MAX_;
    }
    __syncthreads();
    const bool active = lane * PER < D, last_lane = (lane + 1) * PER >= D;
    const size_t base = pair * g.cells + (size_t)y * W1 * D + lane * PER;
    const int16_t *__restrict__ Cp = C + base;
    const PlaneT *__restrict__ Pp[4] = {planes + base, planes + g.plane_stride + base, planes + 2 * g.plane_stride + base,
                                         planes + 3 * g.plane_stride + base};
    int Lp[PER], L[PER], Cv[PER], Cn[PER], Sf[PER], Sn[PER];
#pragma unroll
    for (int k = 0; k < PER; k++)
        Lp[k] = 0;
    int minLp = 0;
    auto load_s = [&](int x, int (&s)[PER]) {
#pragma unroll
        for (int k = 0; k < PER; k++) {
            const size_t o = (size_t)x * D + k;
            s[k] = active ? sat16(Pp[0][o] + Pp[1][o] + Pp[2][o] + Pp[3][o]) : 0;   // R7: one saturation of the sweep's sum
        }
    };
    if (W1 > 0) {
        load_c<PER>(Cp + (size_t)(W1 - 1) * D, active, Cn);
        load_s(W1 - 1, Sn);
    }
    for (int x = W1 - 1; x >= 0; x--) {
#pragma unroll
        for (int k = 0; k < PER; k++)
            Cv[k] = Cn[k], Sf[k] = Sn[k];
        if (x > 0) {
            load_c<PER>(Cp + (size_t)(x - 1) * D, active, Cn);
            load_s(x - 1, Sn);
        }
        path_step<PER>(Cv, Lp, minLp, L, last_lane, g.P1, g.P2);
        int mn = INT_MAX, key = INT_MAX;
#pragma unroll
        for (int k = 0; k < PER; k++) {
            mn = min(mn, L[k]);
            Lp[k] = (int16_t)L[k];
            const int s = sat16(Sf[k] + L[k]);
            Sf[k] = s;
            if (active) {
                srow[lane * PER + k] = s;
                key = min(key, s * 512 + lane * PER + k);   // the first d of the smallest S
            }
        }
        minLp = (int16_t)svo::wave_min(active ? mn : INT_MAX);
        key = svo::wave_min(key);
        int minS = key >> 9, best = key & 511;
        if (minS >= SHORT_MAX_)   // strict < from SHRT_MAX: nothing below it -> d = -1 (R7)
            minS = SHORT_MAX_, best = -1;
        bool bad = false;
#pragma unroll
        for (int k = 0; k < PER; k++) {
            const int d = lane * PER + k;
            bad |= active && Sf[k] * (100 - g.ratio) < minS * 100 && abs(best - d) > 1;
        }
        __syncthreads();
        if (__any(bad)) {
            __syncthreads();
            continue;
        }
        if (lane == 0) {
            int d = best;
            const int x2 = x + minX1 - d - minD;
            if (x2 >= 0 && x2 < w && cost2[x2] > minS) {
                cost2[x2] = minS;
                disp2[x2] = (int16_t)(d + minD);
            }
            if (0 < d && d < D - 1) {
                const int sm = srow[d - 1], s0 = srow[d], sp = srow[d + 1];
                const int denom2 = max(sm + sp - 2 * s0, 1);
                d = d * 16 + ((sm - sp) * 16 + denom2) / (denom2 * 2);   // C division: truncation toward zero (R10)
            } else {
                d *= 16;
            }
            drow[x + minX1] = (int16_t)(d + minD * 16);
        }
        __syncthreads();
    }
    __syncthreads();
    int16_t *__restrict__ out = raw + (size_t)pair * g.h * w + (size_t)y * w;
    for (int x = lane; x < w; x += 64) {
        int d1 = drow[x];
        if (x >= minX1 && x < minX1 + W1 && d1 != invalid) {
            const int _d = d1 >> 4, d_ = (d1 + 15) >> 4;
            const int _x = x - _d, x_ = x - d_;
            if (0 <= _x && _x < w && disp2[_x] >= minD && abs(disp2[_x] - _d) > g.maxdiff && 0 <= x_ && x_ < w &&
                disp2[x_] >= minD && abs(disp2[x_] - d_) > g.maxdiff)
                d1 = invalid;
        }
        out[x] = (int16_t)d1;
    }
}

// ---- medianBlur(3), replicated border ----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sgbm_median_kernel(const int16_t *__restrict__ in, int16_t *__restrict__ out, int w, int h,
                                                          int n)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)n * w * h)
        return;
    const int x = (int)(i % w), y = (int)((i / w) % h);
    const int16_t *img = in + (i - (size_t)y * w - x);
    int v[9], k = 0;
    for (int dy = -1; dy <= 1; dy++)
        for (int dx = -1; dx <= 1; dx++) {
            const int yy = min(max(y + dy, 0), h - 1), xx = min(max(x + dx, 0), w - 1);
            v[k++] = img[(size_t)yy * w + xx];
        }
    for (int a = 1; a < 9; a++) {   // insertion sort of nine
        const int t = v[a];
        int b = a - 1;
        while (b >= 0 && v[b] > t) {
            v[b + 1] = v[b];
            b--;
        }
        v[b + 1] = t;
    }
    out[i] = (int16_t)v[4];
}

// ---- filterSpeckles: union-find over 4-neighbours ----------------------------------------------------------------------
__device__ __forceinline__ int uf_find(int *parent, int p)
{
    int q = __hip_atomic_load(parent + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (q != p) {
        p = q;
        q = __hip_atomic_load(parent + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return p;
}

__device__ __forceinline__ void uf_union(int *parent, int a, int b)
{
    for (;;) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b)
            return;
        if (a > b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(parent + b, a);   // hang the larger root under the smaller
        if (old == b)
            return;
        b = old;
    }
}

__global__ __launch_bounds__(256) void speckle_init_kernel(const int16_t *__restrict__ disp, int *__restrict__ parent, int *__restrict__ size,
                                                           int total, int new_val)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total)
        return;
    parent[i] = disp[i] != new_val ? i : -1;
    size[i] = 0;
}

__global__ __launch_bounds__(256) void speckle_link_kernel(const int16_t *__restrict__ disp, int *parent, int w, int h, int total,
                                                           int new_val, int max_diff)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total)
        return;
    const int d = disp[i];
    if (d == new_val)
        return;
    const int x = i % w, y = (i / w) % h;
    if (x + 1 < w) {
        const int e = disp[i + 1];
        if (e != new_val && abs(d - e) <= max_diff)
            uf_union(parent, i, i + 1);
    }
    if (y + 1 < h) {
        const int e = disp[i + w];
        if (e != new_val && abs(d - e) <= max_diff)
            uf_union(parent, i, i + w);
    }
}

// after the links: every pixel points straight at its root (the walk's nodes are pointed there too; no union runs
// concurrently, so every write names an ancestor of the node written)
__global__ __launch_bounds__(256) void speckle_compress_kernel(int *parent, int total)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total || parent[i] < 0)
        return;
    const int r = uf_find(parent, i);
    int p = i;
    while (p != r) {
        const int q = __hip_atomic_load(parent + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(parent + p, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        p = q;
    }
}

// component sizes: one atomicAdd per distinct root of a wave (a large component would otherwise take every pixel's add
// on one address)
__global__ __launch_bounds__(256) void speckle_count_kernel(const int *__restrict__ parent, int *__restrict__ size, int total)
{
    const int i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    const int r = i < total ? parent[i] : -1;
    bool pending = r >= 0;
    while (__any(pending)) {
        const unsigned long long m = __ballot(pending);
        const int leader = __ffsll((unsigned long long)m) - 1;
        const int lr = __shfl(r, leader);
        const bool mine = pending && r == lr;
        const unsigned long long grp = __ballot(mine);
        if (lane == leader)
            atomicAdd(size + lr, __popcll(grp));
        if (mine)
            pending = false;
    }
}

__global__ __launch_bounds__(256) void speckle_apply_kernel(int16_t *__restrict__ disp, const int *__restrict__ parent, const int *__restrict__ size,
                                                            int total, int new_val, int max_size)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total || parent[i] < 0)
        return;
    if (size[parent[i]] <= max_size)
        disp[i] = (int16_t)new_val;
}

// ---- reprojectImageTo3D + the loop of reprojectDisparity --------------------------------------------------------------
struct ReprojArgs {
    double q[16];
    float disp_scale, z_min, z_max;
    int w, h, c, flip_y;
};

__global__ __launch_bounds__(256) void sgbm_reproject_kernel(ReprojArgs a, const int16_t *__restrict__ disp,
                                                             const uint8_t *__restrict__ img, float *__restrict__ xyz,
                                                             float *__restrict__ bgr, uint8_t *__restrict__ mask)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.w * a.h)
        return;
    const int x = i % a.w, y = i / a.w;
    const double *q = a.q;
    const double d = (double)((float)disp[i] * a.disp_scale);
    const double qx = (q[1] * y + q[3]) + q[0] * x, qy = (q[5] * y + q[7]) + q[4] * x;
    const double qz = (q[9] * y + q[11]) + q[8] * x, qw = (q[13] * y + q[15]) + q[12] * x;
    const double iW = 1.0 / (qw + q[14] * d);
    const float X = (float)((qx + q[2] * d) * iW), Y = (float)((qy + q[6] * d) * iW), Z = (float)((qz + q[10] * d) * iW);
    mask[i] = (Z > a.z_max || Z <= a.z_min) ? 0 : 1;   // NaN passes, as the reference's comparison lets it
    xyz[3 * (size_t)i] = X;
    xyz[3 * (size_t)i + 1] = a.flip_y ? -Y : Y;
    xyz[3 * (size_t)i + 2] = Z;
    if (bgr) {
        for (int k = 0; k < 3; k++)
            bgr[3 * (size_t)i + k] = (float)(a.c == 1 ? img[i] : img[3 * (size_t)i + k]);
    }
}

// host: stereoRectify's Q (R15)
void rectify_q(double fx, double fy, double cx, double cy, double tx, int w, int h, double *Q)
{
    const double fc_new = fy, ifx = 1. / fx, ify = 1. / fy;
    const double cu[4] = {0, (double)(w - 1), 0, (double)(w - 1)}, cv[4] = {0, 0, (double)(h - 1), (double)(h - 1)};
    double sx = 0, sy = 0;
    for (int i = 0; i < 4; i++) {
        const float xu = (float)(((double)(float)cu[i] - cx) * ifx), yu = (float)(((double)(float)cv[i] - cy) * ify);
        sx += (double)(float)((double)xu * fc_new + 0.0);
        sy += (double)(float)((double)yu * fc_new + 0.0);
    }
    const double ccx = (w - 1) / 2.0 - sx * 0.25, ccy = (h - 1) / 2.0 - sy * 0.25;
    for (int i = 0; i < 16; i++)
        Q[i] = 0;
    Q[0] = Q[5] = 1.0;
    Q[3] = -ccx;
    Q[7] = -ccy;
    Q[11] = fc_new;
    Q[14] = -1.0 / tx;
    Q[15] = (ccx - ccx) / tx;
}

// Whether some path cost L can leave int16.  While C does not wrap, C lies in [P2, P2 + the largest block sum]; R6 gives
// C - P2 <= L <= C as long as the stored Lr' and minLr' are the true ones, so by induction every L lies in [0, 32767] when
// that upper end does.  A pixel costs at most the largest derivative value (2 ftzero, a uchar: R1) plus 255 >> 2.
bool planes_need_int(const SgbmGeom &g)
{
    const long long side = 2 * g.SW2 + 1, pixmax = (2 * g.ftzero < 255 ? 2 * g.ftzero : 255) + 63;
    return g.P2 + side * side * pixmax > SHORT_MAX_;
}

template <int PER, class PlaneT>
void launch_paths(const SgbmGeom &g, int n_pairs, hipStream_t st, const int16_t *dC, void *planes, int16_t *raw)
{
    const int n_lines = g.h + g.width1 + 2 * (g.width1 + g.h - 1);
    hipLaunchKernelGGL((sgbm_path_kernel<PER, PlaneT>), dim3((n_lines + 3) / 4, n_pairs), dim3(256), 0, st, g, dC,
                       static_cast<PlaneT *>(planes), n_lines);
    hipLaunchKernelGGL((sgbm_wta_kernel<PER, PlaneT>), dim3(g.h, n_pairs), dim3(64), 0, st, g, dC,
                       static_cast<const PlaneT *>(planes), raw);
}

template <int PER> void launch_paths(const SgbmGeom &g, bool wide, int n_pairs, hipStream_t st, const int16_t *dC, void *planes,
                                     int16_t *raw)
{
    if (wide)
        launch_paths<PER, int>(g, n_pairs, st, dC, planes, raw);
    else
        launch_paths<PER, int16_t>(g, n_pairs, st, dC, planes, raw);
}

int sgbm_check(const svo_sgbm_params *p, int w, int h)
{
    SVO_CHECK_ARG(p != nullptr);
    SVO_CHECK_ARG(p->mode == SVO_SGBM_MODE_SGBM);
    SVO_CHECK_ARG(p->num_disparities > 0 && p->num_disparities % 16 == 0 && p->num_disparities <= 256);
    SVO_CHECK_ARG(p->block_size % 2 == 1 && p->block_size >= 1 && p->block_size <= 11);
    SVO_CHECK_ARG(p->p2 > p->p1);
    SVO_CHECK_ARG(h >= 1 && w > p->num_disparities + p->min_disparity);
    return SVO_OK;
}

}  // namespace

// the five launches of filterSpeckles; the caller checks hipGetLastError
int svo_launch_speckle(hipStream_t st, int16_t *disp, int *parent, int *sizes, int w, int h, int n_pairs, int new_val,
                       int max_diff, int max_size)
{
    const int total = n_pairs * w * h;
    const unsigned nb = (unsigned)((total + 255) / 256);
    hipLaunchKernelGGL(speckle_init_kernel, dim3(nb), dim3(256), 0, st, disp, parent, sizes, total, new_val);
    hipLaunchKernelGGL(speckle_link_kernel, dim3(nb), dim3(256), 0, st, disp, parent, w, h, total, new_val, max_diff);
    hipLaunchKernelGGL(speckle_compress_kernel, dim3(nb), dim3(256), 0, st, parent, total);
    hipLaunchKernelGGL(speckle_count_kernel, dim3(nb), dim3(256), 0, st, parent, sizes, total);
    hipLaunchKernelGGL(speckle_apply_kernel, dim3(nb), dim3(256), 0, st, disp, parent, sizes, total, new_val, max_size);
    return SVO_OK;
}

extern "C" {

void svo_sgbm_default_params(svo_sgbm_params *p)
{
    if (!p)
        return;
    p->min_disparity = 1;
    p->num_disparities = 96;
    p->block_size = 7;
    p->p1 = 24;
    p->p2 = 96;
    p->disp12_max_diff = 0;
    p->pre_filter_cap = 60;
    p->uniqueness_ratio = 0;
    p->speckle_window_size = 3000;
    p->speckle_range = 5;
    p->mode = SVO_SGBM_MODE_SGBM;
}

int svo_sgbm_compute(svo_ctx *ctx, const svo_sgbm_params *p, const uint8_t *left, const uint8_t *right, int w, int h, int c,
                     int n_pairs, int16_t *disp, int mem)
{
    int rc;
    if ((rc = sgbm_check(p, w, h)))
        return rc;
    SVO_CHECK_ARG(ctx && left && right && disp);
    SVO_CHECK_ARG(c == 1 || c == 3);
    SVO_CHECK_ARG(n_pairs >= 1 && n_pairs <= SVO_LK_MAX_JOBS);
    SVO_CHECK_ARG(mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE);
    if (w > SGBM_MAXW) {
        svo_set_error("svo_sgbm_compute: images wider than %d pixels", SGBM_MAXW);
        return SVO_ERR_CAPACITY;
    }
    SgbmGeom g;
    g.w = w, g.h = h, g.c = c, g.minD = p->min_disparity, g.D = p->num_disparities;
    const int maxD = g.minD + g.D;
    g.minX1 = maxD > 0 ? maxD : 0;
    g.width1 = w + (g.minD < 0 ? g.minD : 0) - g.minX1;
    g.P1 = p->p1 > 0 ? p->p1 : 2;
    g.P2 = p->p2 > 0 ? p->p2 : 5;
    g.P2 = g.P2 > g.P1 + 1 ? g.P2 : g.P1 + 1;
    g.ftzero = (p->pre_filter_cap > 15 ? p->pre_filter_cap : 15) | 1;
    g.ratio = p->uniqueness_ratio >= 0 ? p->uniqueness_ratio : 10;
    g.maxdiff = p->disp12_max_diff > 0 ? p->disp12_max_diff : 1;
    g.SW2 = g.SH2 = p->block_size / 2;
    g.img_stride = (size_t)w * h * c;
    const int W1 = g.width1 > 0 ? g.width1 : 0;
    g.cells = (size_t)h * W1 * g.D;
    g.plane_stride = g.cells * n_pairs;
    if (g.plane_stride > SGBM_MAX_CELLS) {
        svo_set_error("svo_sgbm_compute: %zu cost cells per call, at most %zu", g.plane_stride, SGBM_MAX_CELLS);
        return SVO_ERR_CAPACITY;
    }
    SVO_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t npix = (size_t)n_pairs * w * h;
    const uint8_t *dl = left, *dr = right;
    int16_t *dout = disp;
    if (mem == SVO_MEM_HOST) {
        if ((rc = ctx->s_a.ensure(g.img_stride * n_pairs)) || (rc = ctx->s_b.ensure(g.img_stride * n_pairs)) ||
            (rc = ctx->s_c.ensure(npix * 2)))
            return rc;
        SVO_HIP(hipMemcpyAsync(ctx->s_a.p, left, g.img_stride * n_pairs, hipMemcpyHostToDevice, st));
        SVO_HIP(hipMemcpyAsync(ctx->s_b.p, right, g.img_stride * n_pairs, hipMemcpyHostToDevice, st));
        dl = ctx->s_a.as<uint8_t>();
        dr = ctx->s_b.as<uint8_t>();
        dout = ctx->s_c.as<int16_t>();
    }
    // scratch, kept in the context and grown on demand: C, four direction planes of int16 or int (hsum lies first where
    // the fourth int16 plane does), the raw disparities, the union-find parents and sizes
    const bool wide = planes_need_int(g);
    if ((rc = ctx->sgbm_cost.ensure(g.plane_stride * (sizeof(int16_t) + 4 * (wide ? sizeof(int) : sizeof(int16_t))) + 256)) ||
        (rc = ctx->sgbm_misc.ensure(npix * (2 + 4 + 4) + 256)))
        return rc;
    int16_t *dC = ctx->sgbm_cost.as<int16_t>(), *planes = dC + g.plane_stride, *hs = planes + 3 * g.plane_stride;
    int16_t *raw = ctx->sgbm_misc.as<int16_t>();
    int *parent = reinterpret_cast<int *>(ctx->sgbm_misc.as<uint8_t>() + ((npix * 2 + 15) / 16) * 16);
    int *sizes = parent + npix;
    if (W1 > 0) {
        hipLaunchKernelGGL(sgbm_hsum_kernel, dim3(h, n_pairs), dim3(256), 0, st, g, dl, dr, hs);
        hipLaunchKernelGGL(sgbm_vsum_kernel, dim3((unsigned)((W1 * g.D + 255) / 256), n_pairs), dim3(256), 0, st, g, hs, dC);
        if (g.D <= 64)
            launch_paths<1>(g, wide, n_pairs, st, dC, planes, raw);
        else if (g.D <= 128)
            launch_paths<2>(g, wide, n_pairs, st, dC, planes, raw);
        else
            launch_paths<4>(g, wide, n_pairs, st, dC, planes, raw);
    } else {   // an empty band: every pixel invalid (3.2 returns early; the median keeps a constant image)
        hipLaunchKernelGGL((sgbm_wta_kernel<1, int16_t>), dim3(h, n_pairs), dim3(64), 0, st, g, dC, planes, raw);
    }
    const unsigned nb = (unsigned)((npix + 255) / 256);
    hipLaunchKernelGGL(sgbm_median_kernel, dim3(nb), dim3(256), 0, st, raw, dout, w, h, n_pairs);
    if (p->speckle_window_size > 0)
        svo_launch_speckle(st, dout, parent, sizes, w, h, n_pairs, (g.minD - 1) * 16, 16 * p->speckle_range,
                           p->speckle_window_size);
    SVO_HIP(hipGetLastError());
    if (mem == SVO_MEM_HOST) {
        SVO_HIP(hipMemcpyAsync(disp, dout, npix * 2, hipMemcpyDeviceToHost, st));
        SVO_HIP(hipStreamSynchronize(st));
    }
    return SVO_OK;
}

int svo_stereo_rectify_q(double fx, double fy, double cx, double cy, double tx, int w, int h, double *Q16)
{
    SVO_CHECK_ARG(Q16 && w > 0 && h > 0 && fx != 0 && fy != 0 && tx != 0);
    rectify_q(fx, fy, cx, cy, tx, w, h, Q16);
    return SVO_OK;
}

int svo_stereo_reproject(svo_ctx *ctx, const int16_t *disp, const uint8_t *image, int w, int h, int c, const double *Q16,
                         float disp_scale, float z_min, float z_max, int flip_y, float *xyz_out, float *bgr_out, int *n_out,
                         int mem)
{
    SVO_CHECK_ARG(ctx && disp && Q16 && xyz_out && n_out);
    SVO_CHECK_ARG(w > 0 && h > 0 && (long long)w * h < (1LL << 28));
    SVO_CHECK_ARG(!bgr_out || (image && (c == 1 || c == 3)));
    SVO_CHECK_ARG(mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE);
    *n_out = 0;
    SVO_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t npix = (size_t)w * h;
    int rc;
    if ((rc = ctx->sgbm_rp.ensure(npix * (12 + 12 + 1) + 64)) || (rc = ctx->s_g.ensure(64)))
        return rc;
    float *txyz = ctx->sgbm_rp.as<float>(), *tbgr = txyz + 3 * npix;
    uint8_t *mask = reinterpret_cast<uint8_t *>(tbgr + 3 * npix);
    int *d_cnt = ctx->s_g.as<int>();
    const int16_t *dd = disp;
    const uint8_t *di = image;
    float *ox = xyz_out, *ob = bgr_out;
    if (mem == SVO_MEM_HOST) {
        if ((rc = ctx->s_a.ensure(npix * 2)) || (rc = ctx->s_b.ensure(npix * 3)) || (rc = ctx->s_c.ensure(npix * 12)) ||
            (rc = ctx->s_d.ensure(npix * 12)))
            return rc;
        SVO_HIP(hipMemcpyAsync(ctx->s_a.p, disp, npix * 2, hipMemcpyHostToDevice, st));
        if (bgr_out)
            SVO_HIP(hipMemcpyAsync(ctx->s_b.p, image, npix * c, hipMemcpyHostToDevice, st));
        dd = ctx->s_a.as<int16_t>();
        di = ctx->s_b.as<uint8_t>();
        ox = ctx->s_c.as<float>();
        ob = ctx->s_d.as<float>();
    }
    ReprojArgs a;
    for (int i = 0; i < 16; i++)
        a.q[i] = Q16[i];
    a.disp_scale = disp_scale, a.z_min = z_min, a.z_max = z_max;
    a.w = w, a.h = h, a.c = c, a.flip_y = flip_y ? 1 : 0;
    hipLaunchKernelGGL(sgbm_reproject_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, st, a, dd, di, txyz,
                       bgr_out ? tbgr : nullptr, mask);
    if ((rc = svo_launch_compact(ctx, mask, (int)npix, nullptr, txyz, 3, ox, bgr_out ? tbgr : nullptr, bgr_out ? 3 : 0,
                                 bgr_out ? ob : nullptr, nullptr, 0, nullptr, d_cnt)))
        return rc;
    SVO_HIP(hipGetLastError());
    SVO_HIP(hipMemcpyAsync(ctx->pinned, d_cnt, 4, hipMemcpyDeviceToHost, st));
    SVO_HIP(hipStreamSynchronize(st));
    const int kept = reinterpret_cast<int *>(ctx->pinned)[0];
    *n_out = kept;
    if (mem == SVO_MEM_HOST && kept > 0) {
        SVO_HIP(hipMemcpyAsync(xyz_out, ox, (size_t)kept * 12, hipMemcpyDeviceToHost, st));
        if (bgr_out)
            SVO_HIP(hipMemcpyAsync(bgr_out, ob, (size_t)kept * 12, hipMemcpyDeviceToHost, st));
        SVO_HIP(hipStreamSynchronize(st));
    }
    return SVO_OK;
}

}  // extern "C"
