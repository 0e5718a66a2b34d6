// bm.hip -- dense stereo by block matching: cv::StereoBM (StereoBM::create(0, 21) + compute).  The recipe and every recalled
// point of it: tests/bm_numpy.py (B1..B11), DESIGN.md section 10q.  Integer arithmetic throughout; the results are bit-identical
// to the restatement.  Every sizing decision is bm_plan.hip.h's.
//
// Per call (n pairs; blockIdx.z or .y = pair; one launch per stage):
//   bm_prefilter_kernel  one thread per pixel of both images of every pair: grey (cv_gray weights), XSOBEL (B2) -> uint8 planes;
//                        the left images' threads also write FILTERED outside the band (B3)
//   bm_match_kernel      one workgroup per (tile of tx band columns, band of BAND rows): SAD, texture, winner, uniqueness,
//                        sub-pixel (B4..B8), and nothing but the int16 disparity (and minsad, when B9 wants it) leaves it.
//                        A window term depends on (row, u = x + j, d) only, so the workgroup keeps the vertical sums
//                        colsum[u][d] of the current row in LDS, running down the band: per row it stages the entering and
//                        the leaving pre-filtered row (clamps applied while staging), adds / subtracts their terms, forms
//                        the horizontal window sums by one thread per (d, segment of columns) sliding over x, and reduces
//                        over d with THREADS / tx lanes per column (key = sad * 512 + d: the first smallest)
//   bm_validate_kernel   validateDisparity (B9), one workgroup per row: cost2 / disp2 as an atomicMin on cost << 11 | x in
//                        LDS (the smallest cost, the leftmost pixel on ties: what the sequential strict '>' leaves)
//   speckle_*_kernel     sgbm.hip's filterSpeckles (svo_launch_speckle)
#include "svo_internal.h"
#include "bm_plan.hip.h"

#include <climits>

namespace {

struct BmGeom {
    int w, h, c, n_pairs, D, minD, r, lofs, rofs, width1, xe, tx, cap, tex, ratio, filtered, write_cost;
    int ue, rw, sad_stride;                       // bm_plan::Lds
    unsigned o_colsum, o_sad, o_tcol, o_rows;
};

// ---- grey + XSOBEL (B2) ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int bm_grey(const uint8_t *__restrict__ img, int c, size_t i)
{
    if (c == 1)
        return img[i];
    const uint8_t *p = img + 3 * i;
    return svo_bgr2gray(p[0], p[1], p[2]);
}

// images: n_img pointers' worth laid out as [left 0 .. n-1] and [right 0 .. n-1] through (left, right, n_left); disp (may be
// null): the left images' threads write `filtered` outside band columns [lofs, lofs + xe)
__global__ __launch_bounds__(256) void bm_prefilter_kernel(const uint8_t *__restrict__ left, const uint8_t *__restrict__ right,
                                                           int n_left, int w, int h, int c, int cap, uint8_t *__restrict__ out,
                                                           int16_t *__restrict__ disp, int lofs, int xe, int filtered)
{
    const size_t npix = (size_t)w * h;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int img = blockIdx.y;
    if (i >= npix)
        return;
    const int x = (int)(i % w), y = (int)(i / w);
    const uint8_t *__restrict__ src = img < n_left ? left + (size_t)img * npix * c : right + (size_t)(img - n_left) * npix * c;
    int v = cap;
    // the pair loop covers rows 0 .. (h & ~1) - 1; an odd height's last row keeps ftzero
    if (y < (h & ~1) && x >= 1 && x < w - 1) {
        const int ya = y > 0 ? y - 1 : (h > 1 ? 1 : 0), yb = y < h - 1 ? y + 1 : (h > 1 ? y - 1 : y);
        const size_t ra = (size_t)ya * w + x, rb = (size_t)y * w + x, rc = (size_t)yb * w + x;
        const int s = (bm_grey(src, c, ra + 1) - bm_grey(src, c, ra - 1)) + 2 * (bm_grey(src, c, rb + 1) - bm_grey(src, c, rb - 1)) +
                      (bm_grey(src, c, rc + 1) - bm_grey(src, c, rc - 1));
        v = min(max(s, -cap), cap) + cap;
    }
    out[(size_t)img * npix + i] = (uint8_t)v;
    if (disp && img < n_left && (x < lofs || x >= lofs + xe))
        disp[(size_t)img * npix + i] = (int16_t)filtered;
}

// one 8-bit absolute difference added to acc: v_sad_u8 on dwords whose upper bytes are zero
__device__ __forceinline__ unsigned absdiff_acc(unsigned a, unsigned b, unsigned acc) { return __builtin_amdgcn_sad_u8(a, b, acc); }

// ---- SAD, texture, winner, uniqueness, sub-pixel (B4..B8) ----------------------------------------------------------------
__global__ __launch_bounds__(bm_plan::THREADS) void bm_match_kernel(BmGeom g, const uint8_t *__restrict__ pf, int16_t *__restrict__ disp,
                                                                    int *__restrict__ cost)
{
    extern __shared__ __align__(16) uint8_t lds[];
    uint16_t *colsum = reinterpret_cast<uint16_t *>(lds + g.o_colsum);
    int *sadrow = reinterpret_cast<int *>(lds + g.o_sad);
    int *tcol = reinterpret_cast<int *>(lds + g.o_tcol);
    uint8_t *le = lds + g.o_rows, *ll = le + g.ue, *re = ll + g.ue, *rl = re + g.rw;

    const int t = threadIdx.x, pair = blockIdx.z;
    const int x0 = blockIdx.x * g.tx, y0 = blockIdx.y * bm_plan::BAND;
    const int w = g.w, h = g.h, D = g.D, r = g.r, ue = g.ue, rw = g.rw, tx = g.tx;
    const size_t npix = (size_t)w * h;
    const uint8_t *__restrict__ Lp = pf + (size_t)pair * npix;
    const uint8_t *__restrict__ Rp = pf + (size_t)(g.n_pairs + pair) * npix;
    // B4's clamps, applied while staging: left column of u, right column of (u, d = 0) relative to the strip's first
    const int ub0 = x0 - r;                                                    // band column of u = 0
    const int cmin = g.rofs + min(max(ub0, -g.rofs), g.width1 - 1);            // the strip's first right-image column

    for (int e = t; e < ue * D; e += bm_plan::THREADS)
        colsum[e] = 0;
    for (int e = t; e < ue; e += bm_plan::THREADS)
        tcol[e] = 0;

    const int rows = min(bm_plan::BAND, h - y0), steps = rows + 2 * r;
    const int dl = t & 15, ul = t >> 4;
    const int tpx = bm_plan::THREADS / tx, xq = t / tpx, q = t % tpx;          // reduction: tpx lanes per column
    const int nseg = max(1, bm_plan::THREADS / D), seglen = (tx + nseg - 1) / nseg;
    const int sd = t % D, sg = t / D;                                          // horizontal sums: one thread per (d, segment)
    for (int s = 0; s < steps; s++) {
        const int ye = min(max(y0 - r + s, 0), h - 1);
        const bool sub = s >= 2 * r + 1;
        const int yl = min(max(y0 - r + s - (2 * r + 1), 0), h - 1);
        __syncthreads();   // the rows and colsum of the step before have been read
        for (int u = t; u < ue; u += bm_plan::THREADS) {
            const int cl = min(max(g.lofs + ub0 + u, 0), w - 1);
            le[u] = Lp[(size_t)ye * w + cl];
            ll[u] = Lp[(size_t)yl * w + cl];
        }
        for (int k = t; k < rw; k += bm_plan::THREADS) {
            const int cr = min(cmin + k, w - 1);
            re[k] = Rp[(size_t)ye * w + cr];
            rl[k] = Rp[(size_t)yl * w + cr];
        }
        __syncthreads();
        for (int u = ul; u < ue; u += 16) {
            const unsigned a = le[u], b = ll[u];
            const int ro = g.rofs + min(max(ub0 + u, -g.rofs), g.width1 - 1) - cmin;   // in [0, ue)
            for (int d = dl; d < D; d += 16) {
                unsigned cs = absdiff_acc(a, re[ro + d], colsum[u * D + d]);
                if (sub)
                    cs -= absdiff_acc(b, rl[ro + d], 0u);
                colsum[u * D + d] = (uint16_t)cs;
            }
        }
        if (t < ue) {
            int ts = tcol[t] + abs((int)le[t] - g.cap);
            if (sub)
                ts -= abs((int)ll[t] - g.cap);
            tcol[t] = ts;
        }
        if (s < 2 * r)   // uniform: the window of the band's first row is not complete yet
            continue;
        const int y = y0 + s - 2 * r;
        __syncthreads();
        if (sg < nseg) {
            const int xs = sg * seglen, xend = min(xs + seglen, tx);
            if (xs < xend) {
                int sum = 0;
                for (int k = 0; k <= 2 * r; k++)
                    sum += colsum[(xs + k) * D + sd];
                sadrow[xs * g.sad_stride + sd] = sum;
                for (int x = xs + 1; x < xend; x++) {
                    sum += (int)colsum[(x + 2 * r) * D + sd] - (int)colsum[(x - 1) * D + sd];
                    sadrow[x * g.sad_stride + sd] = sum;
                }
            }
        }
        __syncthreads();
        // every lane takes part in the shuffles; xq < tx always (THREADS = tx * tpx)
        const int *srow = sadrow + xq * g.sad_stride;
        int key = INT_MAX;
        for (int d = q; d < D; d += tpx)
            key = min(key, srow[d] * 512 + d);            // the first d of the smallest SAD (B6)
        for (int o = 1; o < tpx; o <<= 1)
            key = min(key, __shfl_xor(key, o));
        const int minsad = key >> 9, mind = key & 511;
        int bad = 0;
        if (g.ratio > 0) {
            const long long thresh = minsad + (long long)minsad * g.ratio / 100;   // B7
            for (int d = q; d < D; d += tpx)
                bad |= (d < mind - 1 || d > mind + 1) && srow[d] <= thresh;
            for (int o = 1; o < tpx; o <<= 1)
                bad |= __shfl_xor(bad, o);
        }
        if (q == 0 && x0 + xq < g.xe) {
            int tsum = 0;
            for (int k = 0; k <= 2 * r; k++)
                tsum += tcol[xq + k];
            int val = g.filtered;
            if (tsum >= g.tex && !bad) {
                const int p = srow[mind + 1 < D ? mind + 1 : D - 2], n = srow[mind >= 1 ? mind - 1 : 1];   // B8
                const int den = p + n - 2 * minsad + abs(p - n);
                val = ((D - mind - 1 + g.minD) * 256 + (den != 0 ? (p - n) * 256 / den : 0) + 15) >> 4;
            }
            const size_t o = (size_t)pair * npix + (size_t)y * w + g.lofs + x0 + xq;
            disp[o] = (int16_t)val;
            if (g.write_cost)
                cost[o] = minsad;
        }
    }
}

// ---- validateDisparity (B9): one workgroup per row ------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bm_validate_kernel(int16_t *__restrict__ disp, const int *__restrict__ cost, int w, int h, int minX1,
                                                          int maxX1, int filtered, int lim)
{
    __shared__ int16_t drow[bm_plan::MAX_W];
    __shared__ unsigned best[bm_plan::MAX_W];   // cost << 11 | x of the pixel that owns the right-image column
    const int y = blockIdx.x, pair = blockIdx.y, t = threadIdx.x;
    const size_t base = ((size_t)pair * h + y) * w;
    for (int x = t; x < w; x += 256) {
        drow[x] = disp[base + x];
        best[x] = 0xffffffffu;
    }
    __syncthreads();
    for (int x = minX1 + t; x < maxX1; x += 256) {
        const int d = drow[x];
        if (d == filtered)
            continue;
        const int x2 = x - ((d + 8) >> 4);
        if (x2 >= 0 && x2 < w)
            atomicMin(&best[x2], ((unsigned)cost[base + x] << 11) | (unsigned)x);
    }
    __syncthreads();
    for (int x = minX1 + t; x < maxX1; x += 256) {
        const int d = drow[x];
        if (d == filtered)
            continue;
        const int xa = x - (d >> 4), xb = x - ((d + 15) >> 4);
        if (xa < 0 || xa >= w || xb < 0 || xb >= w)
            continue;
        const unsigned ka = best[xa], kb = best[xb];
        if (ka == 0xffffffffu || kb == 0xffffffffu)   // disp2 still FILTERED
            continue;
        // an owner is never FILTERED, and FILTERED lies below every disparity of the band: disp2 > FILTERED holds
        const int da = drow[ka & 2047], db = drow[kb & 2047];
        if (abs(da - d) > lim && abs(db - d) > lim)
            disp[base + x] = (int16_t)filtered;
    }
}

int bm_fail(const char *fn, int code, const char *why)
{
    svo_set_error("%s: %s", fn, why);
    return code == 1 ? SVO_ERR_ARG : SVO_ERR_CAPACITY;
}

}  // namespace

extern "C" {

void svo_bm_default_params(svo_bm_params *p)
{
    if (!p)
        return;
    p->pre_filter_type = SVO_BM_PREFILTER_XSOBEL;
    p->pre_filter_size = 9;
    p->pre_filter_cap = 31;
    p->block_size = 21;
    p->min_disparity = 0;
    p->num_disparities = 64;
    p->texture_threshold = 10;
    p->uniqueness_ratio = 15;
    p->speckle_window_size = 0;
    p->speckle_range = 0;
    p->disp12_max_diff = -1;
}

int svo_bm_compute(svo_ctx *ctx, const svo_bm_params *p, const uint8_t *left, const uint8_t *right, int w, int h, int c,
                   int n_pairs, int16_t *disp, int mem)
{
    const char *why = nullptr;
    int rc;
    if ((rc = bm_plan::check(p, w, h, c, n_pairs, &why)))
        return bm_fail("svo_bm_compute", rc, why);
    SVO_CHECK_ARG(ctx && left && right && disp);
    SVO_CHECK_ARG(mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE);
    const bm_plan::Geom bg = bm_plan::geometry(w, p->min_disparity, p->num_disparities);
    const bool validate = bm_plan::wants_validate(p), speckle = bm_plan::wants_speckle(p);
    const bm_plan::Scratch S = bm_plan::scratch(w, h, n_pairs, validate, speckle);
    const int tx = bm_plan::tile_width(p->num_disparities, p->block_size);
    const bm_plan::Lds L = bm_plan::lds(tx, p->num_disparities, p->block_size);
    if (L.total > bm_plan::LDS_BUDGET) {
        svo_set_error("svo_bm_compute: %zu bytes of LDS per workgroup", L.total);
        return SVO_ERR_CAPACITY;
    }
    SVO_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t npix = (size_t)n_pairs * w * h, img_bytes = npix * c;
    const uint8_t *dl = left, *dr = right;
    int16_t *dout = disp;
    if (mem == SVO_MEM_HOST) {
        if ((rc = ctx->s_a.ensure(img_bytes)) || (rc = ctx->s_b.ensure(img_bytes)) || (rc = ctx->s_c.ensure(npix * 2)))
            return rc;
        SVO_HIP(hipMemcpyAsync(ctx->s_a.p, left, img_bytes, hipMemcpyHostToDevice, st));
        SVO_HIP(hipMemcpyAsync(ctx->s_b.p, right, img_bytes, hipMemcpyHostToDevice, st));
        dl = ctx->s_a.as<uint8_t>();
        dr = ctx->s_b.as<uint8_t>();
        dout = ctx->s_c.as<int16_t>();
    }
    if ((rc = ctx->bm_work.ensure(S.total + 256)))
        return rc;
    uint8_t *wk = ctx->bm_work.as<uint8_t>();
    uint8_t *pf = wk + S.pf;
    int *cost = reinterpret_cast<int *>(wk + S.cost);
    const int filtered = (p->min_disparity - 1) * 16;
    const unsigned nb = (unsigned)(((size_t)w * h + 255) / 256);
    hipLaunchKernelGGL(bm_prefilter_kernel, dim3(nb, 2 * n_pairs), dim3(256), 0, st, dl, dr, n_pairs, w, h, c, p->pre_filter_cap, pf,
                       dout, bg.lofs, bg.xe, filtered);
    if (!bg.empty) {
        BmGeom g;
        g.w = w, g.h = h, g.c = c, g.n_pairs = n_pairs, g.D = p->num_disparities, g.minD = p->min_disparity;
        g.r = p->block_size / 2, g.lofs = bg.lofs, g.rofs = bg.rofs, g.width1 = bg.width1, g.xe = bg.xe, g.tx = tx;
        g.cap = p->pre_filter_cap, g.tex = p->texture_threshold, g.ratio = p->uniqueness_ratio, g.filtered = filtered;
        g.write_cost = validate ? 1 : 0;
        g.ue = L.ue, g.rw = L.rw, g.sad_stride = L.sad_stride;
        g.o_colsum = (unsigned)L.colsum, g.o_sad = (unsigned)L.sad, g.o_tcol = (unsigned)L.tcol, g.o_rows = (unsigned)L.rows;
        const dim3 grid((unsigned)((bg.xe + tx - 1) / tx), (unsigned)((h + bm_plan::BAND - 1) / bm_plan::BAND), n_pairs);
        hipLaunchKernelGGL(bm_match_kernel, grid, dim3(bm_plan::THREADS), L.total, st, g, pf, dout, cost);
        if (validate) {
            const int maxD = p->min_disparity + p->num_disparities;
            const int d12 = p->disp12_max_diff < 65536 ? p->disp12_max_diff : 65536;   // beyond any difference of two int16
            hipLaunchKernelGGL(bm_validate_kernel, dim3(h, n_pairs), dim3(256), 0, st, dout, cost, w, h, maxD > 0 ? maxD : 0,
                               w + (p->min_disparity < 0 ? p->min_disparity : 0), filtered, 16 * d12);
        }
    }
    if (speckle) {
        const int range = p->speckle_range < 65536 ? p->speckle_range : 65536;
        svo_launch_speckle(st, dout, reinterpret_cast<int *>(wk + S.parent), reinterpret_cast<int *>(wk + S.sizes), w, h, n_pairs,
                           filtered, 16 * range, p->speckle_window_size);
    }
    SVO_HIP(hipGetLastError());
    if (mem == SVO_MEM_HOST) {
        SVO_HIP(hipMemcpyAsync(disp, dout, npix * 2, hipMemcpyDeviceToHost, st));
        SVO_HIP(hipStreamSynchronize(st));
    }
    return SVO_OK;
}

int svo_bm_prefilter(svo_ctx *ctx, const uint8_t *image, int w, int h, int c, int cap, uint8_t *out, int mem)
{
    SVO_CHECK_ARG(c == 1 || c == 3);
    SVO_CHECK_ARG(cap >= 1 && cap <= bm_plan::MAX_CAP);
    SVO_CHECK_ARG(w >= 1 && h >= 1);
    SVO_CHECK_ARG(ctx && image && out);
    SVO_CHECK_ARG(mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE);
    if (w > bm_plan::MAX_W || (long long)w * h >= bm_plan::MAX_CELLS) {
        svo_set_error("svo_bm_prefilter: images wider than %d pixels or of 2^30 pixels", bm_plan::MAX_W);
        return SVO_ERR_CAPACITY;
    }
    SVO_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t npix = (size_t)w * h;
    const uint8_t *din = image;
    uint8_t *dout = out;
    int rc;
    if (mem == SVO_MEM_HOST) {
        if ((rc = ctx->s_a.ensure(npix * c)) || (rc = ctx->s_c.ensure(npix)))
            return rc;
        SVO_HIP(hipMemcpyAsync(ctx->s_a.p, image, npix * c, hipMemcpyHostToDevice, st));
        din = ctx->s_a.as<uint8_t>();
        dout = ctx->s_c.as<uint8_t>();
    }
    hipLaunchKernelGGL(bm_prefilter_kernel, dim3((unsigned)((npix + 255) / 256), 1), dim3(256), 0, st, din, din, 1, w, h, c, cap, dout,
                       static_cast<int16_t *>(nullptr), 0, 0, 0);
    SVO_HIP(hipGetLastError());
    if (mem == SVO_MEM_HOST) {
        SVO_HIP(hipMemcpyAsync(out, dout, npix, hipMemcpyDeviceToHost, st));
        SVO_HIP(hipStreamSynchronize(st));
    }
    return SVO_OK;
}

}  // extern "C"
