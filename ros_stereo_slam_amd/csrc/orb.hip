// orb.hip -- binary features for the loop-closure detector on gfx950.
//
// Replaces the cv::ORB::create()->detectAndCompute(img, Mat(), kp, desc) call of
// visualSLAM::checkLoopDetectorStatus (src/optimizationStuff.cpp:49-56): oriented FAST corners
// ranked by their Harris response + rotation-steered binary tests on a smoothed patch.  The
// recipe (stated in full in oracle/orb.c, which this file matches bit for bit): OpenCV's
// fixed-point grey conversion, 3 octaves of the tracker's factor-2 pyramid, FAST-9 (t = 20),
// Harris 7x7 / k = 0.04 on integer gradient sums, 3x3 non-maximum suppression, the strongest
// 286 / 143 / 71 corners per octave, orientation = unit vector of the radius-15 intensity moments,
// 256 tests from a seeded pattern on the 5x5-binomial-smoothed octave.
//
// Kernels per octave (all byte / integer work, HBM-bound, row-contiguous accesses on the padded
// pyramid level so no border arithmetic):
//   blur5            5x5 binomial, thread per pixel
//   fast_harris      thread per pixel: 16-pixel ring -> two 16-bit masks -> nine-contiguous test by
//                    shifts; corners get their Harris response
//   nms + strip count, strip scan, candidate write: order-preserving multi-workgroup compaction
//                    (the scans and ranks are scan_ops.hip.h's)
//   select           one workgroup: k-th largest response by a 32-step bitwise search over the
//                    candidates, ties at the cut in raster order, ballot-scan write
//   describe         ONE WAVEFRONT PER KEYPOINT: disc moments reduced with DPP, the 256 tests 64 at
//                    a time, descriptor words straight from __ballot
#include <cstring>
#include <vector>

#include "svo_internal.h"
#include "scan_ops.hip.h"
#include "wave_ops.hip.h"

namespace {

constexpr int EDGE = 19, HALF_PATCH = 15, STRIP = 1024, NLEV = 3;

// The three octaves go through every stage in ONE launch (blockIdx.z / .y = the octave): 11 launches per image instead of
// 29, on buffers that hold the octaves side by side.  (A launch per stage and octave was 0.46 ms per image, most of it the
// 4-5 us each of two dozen launches that do microseconds of work.)
struct OrbLevels {
    const uint8_t *lvl[NLEV];
    int pitch[NLEV], w[NLEV], h[NLEV], want[NLEV];
    int pix_off[NLEV], strip_off[NLEV], cand_off[NLEV], cand_cap[NLEV];  // where an octave's part of a work buffer begins
    int on[NLEV];                                                         // 0: too small for the border, or nothing wanted
};

__global__ __launch_bounds__(256) void gray_kernel(const uint8_t *__restrict__ img, int n, int c,
                                                   uint8_t *__restrict__ gray)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    gray[i] = c == 1 ? img[i]
                     : (uint8_t)((1868 * img[3 * i] + 9617 * img[3 * i + 1] + 4899 * img[3 * i + 2] + 8192) >> 14);
}

__global__ __launch_bounds__(256) void blur5_kernel(OrbLevels L, uint8_t *__restrict__ out_all)
{
    const int l = blockIdx.z, w = L.w[l], h = L.h[l], pitch = L.pitch[l];
    const uint8_t *__restrict__ lvl = L.lvl[l];
    uint8_t *__restrict__ out = out_all + L.pix_off[l];
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (!L.on[l] || x >= w || y >= h)
        return;
    int s = 0;
#pragma unroll
    for (int j = -2; j <= 2; j++) {
        const uint8_t *r = lvl + (ptrdiff_t)(y + j) * pitch + x;
        const int kj = j == 0 ? 6 : ((j == 1 || j == -1) ? 4 : 1);
        s += kj * (r[-2] + 4 * r[-1] + 6 * r[0] + 4 * r[1] + r[2]);
    }
    out[(size_t)y * w + x] = (uint8_t)((s + 128) >> 8);
}

__device__ __forceinline__ bool nine_contiguous(unsigned m)
{
    const unsigned d = m | (m << 16);
    unsigned r = d;
#pragma unroll
    for (int k = 1; k < 9; k++)
        r &= d >> k;
    return (r & 0xffffu) != 0;
}

__global__ __launch_bounds__(256) void fast_harris_kernel(OrbLevels L, int t, float *__restrict__ R_all,
                                                          uint8_t *__restrict__ corner_all)
{
    const int l = blockIdx.z, w = L.w[l], h = L.h[l], pitch = L.pitch[l];
    const uint8_t *__restrict__ lvl = L.lvl[l];
    float *__restrict__ R = R_all + L.pix_off[l];
    uint8_t *__restrict__ corner = corner_all + L.pix_off[l];
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (!L.on[l] || x >= w || y >= h)
        return;
    const size_t idx = (size_t)y * w + x;
    float resp = 0.f;
    uint8_t is_c = 0;
    if (x >= EDGE && x < w - EDGE && y >= EDGE && y < h - EDGE) {
        const uint8_t *p0 = lvl + (ptrdiff_t)y * pitch + x;
        const int p = p0[0];
        constexpr int CX[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
        constexpr int CY[16] = {-3, -3, -2, -1, 0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3};
        unsigned br = 0, dk = 0;
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const int q = p0[CY[k] * pitch + CX[k]];
            br |= (q > p + t ? 1u : 0u) << k;
            dk |= (q < p - t ? 1u : 0u) << k;
        }
        if (nine_contiguous(br) || nine_contiguous(dk)) {
            is_c = 1;
            int a = 0, b = 0, c = 0;
            for (int j = -3; j <= 3; j++) {
                const uint8_t *r = p0 + (ptrdiff_t)j * pitch;
#pragma unroll
                for (int i = -3; i <= 3; i++) {
                    const uint8_t *q = r + i;
                    const int ix = (q[1] - q[-1]) * 2 + (q[-pitch + 1] - q[-pitch - 1]) + (q[pitch + 1] - q[pitch - 1]);
                    const int iy = (q[pitch] - q[-pitch]) * 2 + (q[pitch - 1] - q[-pitch - 1]) + (q[pitch + 1] - q[-pitch + 1]);
                    a += ix * ix;
                    b += iy * iy;
                    c += ix * iy;
                }
            }
            const float fa = (float)a, fb = (float)b, fc = (float)c;
            const float sc = 1.f / (4 * 7 * 255.f);
            const float s4 = sc * sc * sc * sc;
            resp = (fa * fb - fc * fc - 0.04f * (fa + fb) * (fa + fb)) * s4;
        }
    }
    R[idx] = resp;
    corner[idx] = is_c;
}

// 3x3 non-maximum suppression among corners (strictly above the raster-earlier neighbours, at
// least equal to the later ones) + the number of survivors per 1024-pixel strip
__global__ __launch_bounds__(STRIP) void nms_count_kernel(OrbLevels L, const float *__restrict__ R_all,
                                                          const uint8_t *__restrict__ corner_all,
                                                          uint8_t *__restrict__ keep_all, int *__restrict__ strip_count_all)
{
    __shared__ int s_w[16];
    const int l = blockIdx.y, w = L.w[l], h = L.h[l];
    if (!L.on[l] || (int)blockIdx.x * STRIP >= w * h)
        return;
    const float *__restrict__ R = R_all + L.pix_off[l];
    const uint8_t *__restrict__ corner = corner_all + L.pix_off[l];
    uint8_t *__restrict__ keep = keep_all + L.pix_off[l];
    int *__restrict__ strip_count = strip_count_all + L.strip_off[l];
    const int idx = blockIdx.x * STRIP + threadIdx.x;
    bool k = false;
    if (idx < w * h && corner[idx]) {
        const int x = idx % w, y = idx / w;
        const float r = R[idx];
        k = true;
#pragma unroll
        for (int j = -1; j <= 1; j++)
#pragma unroll
            for (int i = -1; i <= 1; i++) {
                if (!i && !j)
                    continue;
                const int n = (y + j) * w + x + i;  // corners keep a 19-pixel margin: always inside
                if (!corner[n])
                    continue;
                const bool earlier = j < 0 || (j == 0 && i < 0);
                if (earlier ? !(r > R[n]) : !(r >= R[n]))
                    k = false;
            }
    }
    if (idx < w * h)
        keep[idx] = k ? 1 : 0;
    int total;
    svo::waves_before<STRIP>((int)__popcll(__ballot(k)), s_w, &total);
    if (threadIdx.x == 0)
        strip_count[blockIdx.x] = total;
}

// exclusive scan of the strip counts (one workgroup; n_strips <= a few thousand): `per` strips a thread, a block scan of the
// threads' sums, the strips again
__global__ __launch_bounds__(1024) void strip_scan_kernel(OrbLevels L, const int *__restrict__ cnt_all,
                                                          int *__restrict__ off_all, int *__restrict__ totals)
{
    __shared__ int s_w[16];
    const int l = blockIdx.x, n = (L.w[l] * L.h[l] + STRIP - 1) / STRIP;
    const int *__restrict__ cnt = cnt_all + L.strip_off[l];
    int *__restrict__ off = off_all + L.strip_off[l];
    int *__restrict__ total = totals + l;
    if (!L.on[l]) {
        if (threadIdx.x == 0)
            *total = 0;
        return;
    }
    const int t = threadIdx.x;
    const int per = (n + 1023) / 1024;
    int s = 0;
    for (int i = t * per; i < (t + 1) * per && i < n; i++)
        s += cnt[i];
    int all;
    int acc = svo::block_excl_scan<1024>(s, s_w, &all);
    if (t == 0)
        *total = all;
    for (int i = t * per; i < (t + 1) * per && i < n; i++) {
        off[i] = acc;
        acc += cnt[i];
    }
}

__global__ __launch_bounds__(STRIP) void cand_write_kernel(OrbLevels L, const uint8_t *__restrict__ keep_all,
                                                           const float *__restrict__ R_all, const int *__restrict__ off_all,
                                                           int *__restrict__ cand_idx_all, float *__restrict__ cand_resp_all)
{
    __shared__ int s_w[16];
    const int l = blockIdx.y, n_pix = L.w[l] * L.h[l], cap = L.cand_cap[l];
    if (!L.on[l] || (int)blockIdx.x * STRIP >= n_pix)
        return;
    const uint8_t *__restrict__ keep = keep_all + L.pix_off[l];
    const float *__restrict__ R = R_all + L.pix_off[l];
    const int *__restrict__ off = off_all + L.strip_off[l];
    int *__restrict__ cand_idx = cand_idx_all + L.cand_off[l];
    float *__restrict__ cand_resp = cand_resp_all + L.cand_off[l];
    const int idx = blockIdx.x * STRIP + threadIdx.x;
    const bool k = idx < n_pix && keep[idx];
    const unsigned long long bal = __ballot(k);
    const int base = off[blockIdx.x] + svo::waves_before<STRIP>((int)__popcll(bal), s_w, (int *)nullptr);
    if (k) {
        const int pos = base + svo::lanes_below(bal);
        if (pos < cap) {
            cand_idx[pos] = idx;
            cand_resp[pos] = R[idx];
        }
    }
}

__device__ __forceinline__ unsigned sortable(float f)
{
    const unsigned b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// the `want` strongest candidates (ties at the cut: earlier pixel first), written in raster order
__global__ __launch_bounds__(1024) void select_kernel(OrbLevels L, const int *__restrict__ cand_idx_all,
                                                      const float *__restrict__ cand_resp_all,
                                                      const int *__restrict__ d_nc_all, int n_features,
                                                      int *__restrict__ sel_idx_all, float *__restrict__ sel_resp_all,
                                                      int *__restrict__ d_nsel_all)
{
    __shared__ int s_red[16], s_base, s_ties;
    const int l = blockIdx.x, cap = L.cand_cap[l], want = L.want[l];
    const int *__restrict__ cand_idx = cand_idx_all + L.cand_off[l];
    const float *__restrict__ cand_resp = cand_resp_all + L.cand_off[l];
    int *__restrict__ sel_idx = sel_idx_all + (size_t)l * n_features;
    float *__restrict__ sel_resp = sel_resp_all + (size_t)l * n_features;
    int *__restrict__ d_nsel = d_nsel_all + l;
    if (!L.on[l]) {
        if (threadIdx.x == 0)
            *d_nsel = 0;
        return;
    }
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int nc = min(d_nc_all[l], cap);
    // the want-th largest key, a byte at a time from the top: a 256-bin count of the keys that match the bytes found so
    // far, then the bin the want-th largest falls into (a suffix sum over the bins by 256 threads).  Four rounds of one
    // pass over the candidates; the search bit by bit was 32 passes with three barriers each (37 us of an image's 130).
    __shared__ int s_hist[256], s_pick, s_left;
    unsigned thr = 0;  // everything is >= 0
    int n_above = 0;
    if (nc > want) {
        int left = want;  // how many of the keys that match the prefix are still wanted
        for (int shift = 24; shift >= 0; shift -= 8) {
            if (t < 256)
                s_hist[t] = 0;
            __syncthreads();
            const unsigned himask = shift == 24 ? 0u : 0xffffffffu << (shift + 8);
            for (int i = t; i < nc; i += 1024) {
                const unsigned k = sortable(cand_resp[i]);
                if ((k & himask) == (thr & himask))
                    atomicAdd(&s_hist[(k >> shift) & 255u], 1);
            }
            __syncthreads();
            // above[t] = keys in the bins over t (a suffix sum: shuffles inside each of the four waves, their totals
            // across); the pick is the bin with above < left <= above + count
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
        n_above = want - left;  // `left` of the keys equal to thr make up the rest
    }
    const int ties_allowed = nc > want ? want - n_above : 0;
    if (t == 0) {
        s_base = 0;
        s_ties = 0;
    }
    __syncthreads();
    for (int start = 0; start < nc; start += 1024) {
        const int i = start + t;
        const unsigned key = i < nc ? sortable(cand_resp[i]) : 0u;
        const bool above = i < nc && (nc <= want || key > thr);
        const bool tie = i < nc && nc > want && key == thr;
        // ties first get their running rank (raster order), the first `ties_allowed` are kept
        const unsigned long long tb = __ballot(tie);
        int tie_total, kept_total;
        const int tie_rank = s_ties + svo::waves_before<1024>((int)__popcll(tb), s_red, &tie_total) + svo::lanes_below(tb);
        const bool keep = above || (tie && tie_rank < ties_allowed);
        __syncthreads();  // s_red is read
        const unsigned long long kb = __ballot(keep);
        const int pos = s_base + svo::waves_before<1024>((int)__popcll(kb), s_red, &kept_total) + svo::lanes_below(kb);
        if (keep) {
            sel_idx[pos] = cand_idx[i];
            sel_resp[pos] = cand_resp[i];
        }
        __syncthreads();
        if (t == 0) {
            s_base += kept_total;
            s_ties += tie_total;
        }
        __syncthreads();
    }
    if (t == 0)
        *d_nsel = s_base;
}

// one wavefront per selected keypoint: orientation + descriptor, appended at out_base
__global__ __launch_bounds__(256) void describe_kernel(OrbLevels L, const uint8_t *__restrict__ blur_all,
                                                       const int *__restrict__ sel_idx_all,
                                                       const float *__restrict__ sel_resp_all,
                                                       const int *__restrict__ d_nsel_all, int n_features,
                                                       const int8_t *__restrict__ pat, int *__restrict__ d_total,
                                                       float *__restrict__ xy, int *__restrict__ oct,
                                                       float *__restrict__ resp, float *__restrict__ dir,
                                                       uint32_t *__restrict__ desc)
{
    const int lane = threadIdx.x & 63, octave = blockIdx.y;
    // an octave's features follow those of the octaves before it; the first thread of the launch leaves the total
    int out_base = 0, total = 0;
#pragma unroll
    for (int q = 0; q < NLEV; q++) {
        const int nq = d_nsel_all[q];
        out_base += q < octave ? nq : 0;
        total += nq;
    }
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0)
        *d_total = total;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= d_nsel_all[octave])
        return;
    const uint8_t *__restrict__ lvl = L.lvl[octave];
    const int pitch = L.pitch[octave], w = L.w[octave];
    const uint8_t *__restrict__ blur = blur_all + L.pix_off[octave];
    const int *__restrict__ sel_idx = sel_idx_all + (size_t)octave * n_features;
    const float *__restrict__ sel_resp = sel_resp_all + (size_t)octave * n_features;
    const int idx = sel_idx[i], x = idx % w, y = idx / w;
    int m10 = 0, m01 = 0;
    // the radius-15 disc, row by row; lanes take its 709 pixels in raster order
    for (int e = lane; e < 31 * 31; e += 64) {
        const int v = e / 31 - HALF_PATCH, u = e % 31 - HALF_PATCH;
        if (u * u + v * v <= HALF_PATCH * HALF_PATCH) {  // == |u| <= floor(sqrt(225 - v*v))
            const int p = lvl[(ptrdiff_t)(y + v) * pitch + x + u];
            m10 += u * p;
            m01 += v * p;
        }
    }
    m10 = svo::wave_sum(m10);
    m01 = svo::wave_sum(m01);
    const float f10 = (float)m10, f01 = (float)m01;
    const float nrm = sqrtf(f10 * f10 + f01 * f01);
    const float cs = nrm > 0.f ? f10 / nrm : 1.f, sn = nrm > 0.f ? f01 / nrm : 0.f;
    const int o = out_base + i;
    uint32_t *d = desc + (size_t)8 * o;
#pragma unroll
    for (int pass = 0; pass < 4; pass++) {
        const int b = pass * 64 + lane;
        const float x1 = (float)pat[4 * b], y1 = (float)pat[4 * b + 1], x2 = (float)pat[4 * b + 2],
                    y2 = (float)pat[4 * b + 3];
        const int ax = (int)rintf(cs * x1 - sn * y1), ay = (int)rintf(sn * x1 + cs * y1);
        const int bx = (int)rintf(cs * x2 - sn * y2), by = (int)rintf(sn * x2 + cs * y2);
        const int pa = blur[(size_t)(y + ay) * w + x + ax], pb = blur[(size_t)(y + by) * w + x + bx];
        const unsigned long long bits = __ballot(pa < pb);
        if (lane == 0) {
            d[2 * pass] = (uint32_t)bits;
            d[2 * pass + 1] = (uint32_t)(bits >> 32);
        }
    }
    if (lane == 0) {
        xy[2 * o] = (float)(x << octave);
        xy[2 * o + 1] = (float)(y << octave);
        oct[o] = octave;
        resp[o] = sel_resp[i];
        dir[2 * o] = cs;
        dir[2 * o + 1] = sn;
    }
}


void orb_pattern_host(int8_t *pat)
{
    // the seeded generator stated in oracle/orb.c (three uniforms in [-13, 13], halved)
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

}  // namespace

struct svo_orb {
    svo_ctx *ctx = nullptr;
    int w = 0, h = 0, c = 0, n_features = 500, fast_t = 20;
    svo_pyramid *pyr = nullptr;  // grey, 3 octaves
    DevBuf gray, blur, R, corner, keep, strip_cnt, strip_off, cand_idx, cand_resp, sel_idx, sel_resp, pat, counts;
    OrbLevels lv;            // the octaves' geometry and their places in the work buffers
    int max_strips = 0, max_want = 0;
};

int svo_orb_create(svo_ctx *ctx, int w, int h, int c, int n_features, int fast_t, svo_orb **out)
{
    SVO_CHECK_ARG(ctx && out && w > 4 * EDGE && h > 4 * EDGE && (c == 1 || c == 3) && n_features > 0 && fast_t > 0);
    svo_orb *o = new svo_orb();
    o->ctx = ctx;
    o->w = w;
    o->h = h;
    o->c = c;
    o->n_features = n_features;
    o->fast_t = fast_t;
    int rc = svo_pyramid_create(ctx, w, h, 1, NLEV, &o->pyr);
    if (rc) {
        svo_orb_destroy(o);
        return rc;
    }
    OrbLevels &L = o->lv;
    const PyrDev &pd = o->pyr->dev;
    L.want[0] = (int)(n_features * 4.0 / 7.0 + 0.5);
    L.want[1] = (int)(n_features * 2.0 / 7.0 + 0.5);
    L.want[2] = n_features - L.want[0] - L.want[1];
    size_t pix = 0, strips = 0, cand = 0;
    for (int l = 0; l < NLEV; l++) {
        L.lvl[l] = pd.lvl[l];
        L.pitch[l] = pd.pitch[l];
        L.w[l] = pd.w[l];
        L.h[l] = pd.h[l];
        L.on[l] = L.w[l] > 2 * EDGE && L.h[l] > 2 * EDGE && L.want[l] > 0;
        const size_t npix = (size_t)L.w[l] * L.h[l];
        L.pix_off[l] = (int)pix;
        L.strip_off[l] = (int)strips;
        L.cand_off[l] = (int)cand;
        L.cand_cap[l] = (int)(npix / 4 + 1024);  // non-maximum suppression leaves at most one corner per 2x2
        const int st = (int)((npix + STRIP - 1) / STRIP);
        o->max_strips = st > o->max_strips ? st : o->max_strips;
        o->max_want = L.want[l] > o->max_want ? L.want[l] : o->max_want;
        pix += (npix + 63) & ~(size_t)63;
        strips += st;
        cand += L.cand_cap[l];
    }
    if ((rc = o->gray.ensure((size_t)w * h)) || (rc = o->blur.ensure(pix)) || (rc = o->R.ensure(pix * 4)) ||
        (rc = o->corner.ensure(pix)) || (rc = o->keep.ensure(pix)) || (rc = o->strip_cnt.ensure(strips * 4)) ||
        (rc = o->strip_off.ensure(strips * 4)) || (rc = o->cand_idx.ensure(cand * 4)) ||
        (rc = o->cand_resp.ensure(cand * 4)) || (rc = o->sel_idx.ensure((size_t)NLEV * n_features * 4 + 64)) ||
        (rc = o->sel_resp.ensure((size_t)NLEV * n_features * 4 + 64)) || (rc = o->pat.ensure(1024)) ||
        (rc = o->counts.ensure(64))) {
        svo_orb_destroy(o);
        return rc;
    }
    int8_t pat[1024];
    orb_pattern_host(pat);
    if (hipMemcpy(o->pat.p, pat, sizeof(pat), hipMemcpyHostToDevice) != hipSuccess) {
        svo_set_error("orb: pattern upload failed");
        svo_orb_destroy(o);
        return SVO_ERR_HIP;
    }
    *out = o;
    return SVO_OK;
}

int svo_orb_destroy(svo_orb *o)
{
    if (!o)
        return SVO_OK;
    (void)hipStreamSynchronize(o->ctx->stream);
    if (o->pyr)
        svo_pyramid_destroy(o->ctx, o->pyr);
    DevBuf *bufs[] = {&o->gray, &o->blur, &o->R, &o->corner, &o->keep, &o->strip_cnt, &o->strip_off,
                      &o->cand_idx, &o->cand_resp, &o->sel_idx, &o->sel_resp, &o->pat, &o->counts};
    for (DevBuf *b : bufs)
        b->release();
    delete o;
    return SVO_OK;
}

// d_image: device image (h x w x c).  Device outputs with n_features capacity; *d_n (device int) =
// number of features.  Asynchronous on the context's stream.
int svo_orb_launch(svo_orb *o, const uint8_t *d_image, float *d_xy, int *d_oct, float *d_resp, float *d_dir,
                   uint32_t *d_desc, int *d_n)
{
    svo_ctx *ctx = o->ctx;
    hipStream_t st = ctx->stream;
    const int npix0 = o->w * o->h;
    hipLaunchKernelGGL(gray_kernel, dim3((npix0 + 255) / 256), dim3(256), 0, st, d_image, npix0, o->c,
                       o->gray.as<uint8_t>());
    int rc = svo_build_pyramid_from_device(ctx, o->pyr, o->gray.as<uint8_t>());
    if (rc)
        return rc;
    int *d_nc = o->counts.as<int>(), *d_nsel = d_nc + NLEV;
    const OrbLevels &L = o->lv;
    const dim3 g2((L.w[0] + 255) / 256, L.h[0], NLEV), b2(256);
    hipLaunchKernelGGL(blur5_kernel, g2, b2, 0, st, L, o->blur.as<uint8_t>());
    hipLaunchKernelGGL(fast_harris_kernel, g2, b2, 0, st, L, o->fast_t, o->R.as<float>(), o->corner.as<uint8_t>());
    hipLaunchKernelGGL(nms_count_kernel, dim3(o->max_strips, NLEV), dim3(STRIP), 0, st, L, o->R.as<float>(),
                       o->corner.as<uint8_t>(), o->keep.as<uint8_t>(), o->strip_cnt.as<int>());
    hipLaunchKernelGGL(strip_scan_kernel, dim3(NLEV), dim3(1024), 0, st, L, o->strip_cnt.as<int>(), o->strip_off.as<int>(),
                       d_nc);
    hipLaunchKernelGGL(cand_write_kernel, dim3(o->max_strips, NLEV), dim3(STRIP), 0, st, L, o->keep.as<uint8_t>(),
                       o->R.as<float>(), o->strip_off.as<int>(), o->cand_idx.as<int>(), o->cand_resp.as<float>());
    hipLaunchKernelGGL(select_kernel, dim3(NLEV), dim3(1024), 0, st, L, o->cand_idx.as<int>(), o->cand_resp.as<float>(), d_nc,
                       o->n_features, o->sel_idx.as<int>(), o->sel_resp.as<float>(), d_nsel);
    hipLaunchKernelGGL(describe_kernel, dim3((o->max_want + 3) / 4, NLEV), dim3(256), 0, st, L, o->blur.as<uint8_t>(),
                       o->sel_idx.as<int>(), o->sel_resp.as<float>(), d_nsel, o->n_features, o->pat.as<int8_t>(), d_n, d_xy,
                       d_oct, d_resp, d_dir, d_desc);
    SVO_HIP(hipGetLastError());
    return SVO_OK;
}

extern "C" int svo_orb_extract(svo_ctx *ctx, const uint8_t *image, int w, int h, int c, int n_features,
                               int fast_threshold, float *xy, int *octave, float *response, float *dir,
                               uint32_t *desc, int *n, int mem)
{
    SVO_CHECK_ARG(ctx && image && xy && desc && n && n_features > 0);
    SVO_CHECK_ARG(mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE);
    SVO_HIP(hipSetDevice(ctx->device));
    int rc;
    const int key[5] = {w, h, c, n_features, fast_threshold};
    if (!ctx->orb_cache || memcmp(key, ctx->orb_key, sizeof(key)) != 0) {  // the context keeps one extractor: rebuilt on a new shape
        if (ctx->orb_cache)
            svo_orb_destroy(ctx->orb_cache);
        ctx->orb_cache = nullptr;
        if ((rc = svo_orb_create(ctx, w, h, c, n_features, fast_threshold, &ctx->orb_cache)))
            return rc;
        memcpy(ctx->orb_key, key, sizeof(key));
    }
    svo_orb *o = ctx->orb_cache;
    const size_t nf = (size_t)n_features;
    DevBuf &out = ctx->orb_out;
    const uint8_t *d_img = image;
    if ((rc = out.ensure(nf * (8 + 4 + 4 + 8 + 32) + 64)) ||
        (mem == SVO_MEM_HOST && (rc = ctx->s_img.ensure((size_t)w * h * c))))
        return rc;
    float *dxy = out.as<float>();
    int *doct = reinterpret_cast<int *>(dxy + 2 * nf);
    float *dresp = reinterpret_cast<float *>(doct + nf), *ddir = dresp + nf;
    uint32_t *ddesc = reinterpret_cast<uint32_t *>(ddir + 2 * nf);
    int *dn = reinterpret_cast<int *>(ddesc + 8 * nf);
    hipError_t e = hipSuccess;
    int hn = 0;
    if (mem == SVO_MEM_DEVICE) {
        // straight into the caller's arrays (the ones it does not want: into the context's buffer); one 4-byte copy back
        rc = svo_orb_launch(o, d_img, xy, octave ? octave : doct, response ? response : dresp, dir ? dir : ddir, desc, dn);
        if (!rc) {
            e = hipMemcpyAsync(&hn, dn, 4, hipMemcpyDeviceToHost, ctx->stream);
            if (e == hipSuccess)
                e = hipStreamSynchronize(ctx->stream);
            hn = hn < 0 ? 0 : (hn > n_features ? n_features : hn);   // as the host branch
        }
    } else {
        e = hipMemcpyAsync(ctx->s_img.p, image, (size_t)w * h * c, hipMemcpyHostToDevice, ctx->stream);
        d_img = ctx->s_img.as<uint8_t>();
        if (e == hipSuccess)
            rc = svo_orb_launch(o, d_img, dxy, doct, dresp, ddir, ddesc, dn);
        // the whole record block in ONE copy (28 KB at 500 features), taken apart on the host
        const size_t bytes = nf * (8 + 4 + 4 + 8 + 32) + 4;
        std::vector<unsigned char> &hb = ctx->orb_host;
        if (hb.size() < bytes)
            hb.resize(bytes);
        if (e == hipSuccess && !rc) {
            e = hipMemcpyAsync(hb.data(), out.p, bytes, hipMemcpyDeviceToHost, ctx->stream);
            if (e == hipSuccess)
                e = hipStreamSynchronize(ctx->stream);
        }
        if (e == hipSuccess && !rc) {
            const unsigned char *b = hb.data();
            memcpy(&hn, b + nf * 56, 4);
            hn = hn < 0 ? 0 : (hn > n_features ? n_features : hn);
            memcpy(xy, b, (size_t)hn * 8);
            if (octave)
                memcpy(octave, b + nf * 8, (size_t)hn * 4);
            if (response)
                memcpy(response, b + nf * 12, (size_t)hn * 4);
            if (dir)
                memcpy(dir, b + nf * 16, (size_t)hn * 8);
            memcpy(desc, b + nf * 24, (size_t)hn * 32);
        }
    }
    if (e != hipSuccess) {
        svo_set_error("svo_orb_extract -> %s", hipGetErrorString(e));
        return SVO_ERR_HIP;
    }
    if (rc)
        return rc;
    *n = hn;
    return SVO_OK;
}
