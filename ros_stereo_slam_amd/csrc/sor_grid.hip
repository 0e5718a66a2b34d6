// sor_grid.hip -- statistical outlier removal of large clouds (up to 2^22 points) for gfx950: svo_sor_filter_large.
//
// The algorithm and every rounding step are svo_sor_filter's (sor.hip, oracle/sor.c): the z pre-filter, the mean
// distance to the kk = min(mean_k, m - 1) nearest OTHER points (float squared distances dx*dx + dy*dy + dz*dz, their
// sqrtf summed in double), the cloud statistics in point order, keep d <= mean + mul * stddev.  Points with a
// non-finite coordinate are dropped with the z pre-filter (they must never reach the quantisation below).
//
// What differs is the neighbour search, which sor.hip does by brute force (one wave per point, every distance in VGPRs,
// hence its 9216-point cap):
//   1. bounds of the surviving cloud; every point gets a 63-bit Morton key of its cell on a 2^21 grid per axis;
//   2. (key, index) pairs sorted by a stable LSD radix sort (8-bit digits, 8 passes; the first device sort of the
//      project, its own section below), the points gathered into Morton order;
//   3. a fixed-fan-out box hierarchy over the sorted array: the bounding box of every 64 consecutive points (level 1),
//      of every 64 level-1 boxes (level 2) and of every 64 level-2 boxes (level 3, at most 16 of them for 2^22 points);
//   4. ONE WAVE PER QUERY, queries in Morton order: the query's neighbours in the sorted array seed a per-wave LDS
//      buffer of candidate squared distances (float bits, which order like unsigned ints); the hierarchy is then
//      walked, and a box is skipped only when a lower bound of the float squared distance of any point inside it
//      (computed in double from the query's true coordinates, shrunk by 1e-6 relative, far more than the six
//      roundings of the float expression) is not below the current kk-th smallest candidate.  When the buffer
//      fills, it is cut to its kk smallest values (entries below the kk-th smallest plus copies of it: the multiset of
//      the kk smallest values is all the mean needs, ties cannot change it) and later points are appended only
//      when strictly below that value.  The kk-th smallest is sor.hip's 31-step bitwise search with wave-wide counts.
//   5. the threshold kernel and the compaction, shared with sor.hip.
// Every loop is bounded by construction: 8 sort passes, at most 16 x 64 x 64 level-1 boxes per query, 31 bit steps
// per selection, and a buffer cut frees at least CAP - kk - 64 slots.  Degenerate clouds (all points identical,
// collinear, one far point) only make the boxes overlap more; the walk then visits more of them, never more than all.
//
// Exactness: the multiset of the kk smallest float squared distances of every query is the brute force's, and the
// mean is sum(sqrtf(d) for d < kth) + (kk - count) * sqrtf(kth) in double, as in sor.hip -- the same bits whenever
// that double sum is exact (any realistic spread of distances: float square roots carry 24 significant bits, so
// the sum is exact while the ratio of the largest to the smallest nonzero term stays below 2^29 / kk).
// The keys, the sort, the gather, the box levels and the box bound live in cloud_index.hip.h (shared with cloud.hip).
#include "ransac_common.hip.h"
#include "sor_common.hip.h"
#include "svo_internal.h"
#include "cloud_index.hip.h"

#define SVO_SOR_LARGE_MAX_N (1 << 22)
#define SVO_SOR_LARGE_MAX_K 256

namespace {

// ---- the per-query search ------------------------------------------------------------------------------------------
constexpr int KNN_CAP = 1024;         // candidate squared distances per wave (LDS)
constexpr int KNN_WAVES = 4;          // waves per workgroup

// true when no point of a box whose double lower bound is mind2 can have a float squared distance below r2
__device__ __forceinline__ bool box_skippable(double mind2, unsigned r2)
{
    return mind2 * (1.0 - 1e-6) - 1e-37 >= (double)__uint_as_float(r2);
}

struct KnnWave {
    unsigned *buf;  // KNN_CAP entries of this wave's LDS
    int nb;         // entries held
    bool full;      // the buffer holds exactly the kk smallest seen so far (after a cut); r2 = the largest of them
    unsigned r2;
    int kk, lane;
};

// the kk-th smallest of the buffer: the largest v with count(entry < v) < kk, built bit by bit (as sor.hip)
__device__ unsigned knn_kth(const KnnWave &w)
{
    unsigned kth = 0;
    for (int bit = 30; bit >= 0; bit--) {
        const unsigned test = kth | (1u << bit);
        int c = 0;
        for (int t = w.lane; t < w.nb; t += 64)
            c += w.buf[t] < test ? 1 : 0;
        if (svo::wave_sum_dpp(c) < w.kk)
            kth = test;
    }
    return kth;
}

// cut the buffer (nb >= kk) to its kk smallest values: entries below the kk-th smallest in place, then copies of it
__device__ void knn_cut(KnnWave &w)
{
    const unsigned kth = knn_kth(w);
    int out = 0;
    for (int base = 0; base < w.nb; base += 64) {  // in place: every write lands at or below the chunk just read
        const int t = base + w.lane;
        const unsigned v = t < w.nb ? w.buf[t] : 0xffffffffu;
        const bool keep = t < w.nb && v < kth;
        const unsigned long long bal = __ballot(keep);
        __builtin_amdgcn_wave_barrier();
        if (keep)
            w.buf[out + __popcll(bal & ((1ull << w.lane) - 1ull))] = v;
        __builtin_amdgcn_wave_barrier();
        out += __popcll(bal);
    }
    for (int t = out + w.lane; t < w.kk; t += 64)
        w.buf[t] = kth;
    __builtin_amdgcn_wave_barrier();
    w.nb = w.kk;
    w.full = true;
    w.r2 = kth;
}

// one batch of up to 64 candidates (one per lane)
__device__ __forceinline__ void knn_append(KnnWave &w, bool cand, unsigned d)
{
    bool keep = cand && (!w.full || d < w.r2);
    unsigned long long bal = __ballot(keep);
    if (bal == 0)
        return;
    if (w.nb + __popcll(bal) > KNN_CAP) {  // nb > KNN_CAP - 64 >= kk: a cut leaves kk
        knn_cut(w);
        keep = cand && d < w.r2;
        bal = __ballot(keep);
    }
    if (keep)
        w.buf[w.nb + __popcll(bal & ((1ull << w.lane) - 1ull))] = d;
    __builtin_amdgcn_wave_barrier();
    w.nb += __popcll(bal);
}

__device__ __forceinline__ unsigned dist2_bits(const float *__restrict__ pts, int j, float px, float py, float pz)
{
    const float dx = px - pts[3 * j], dy = py - pts[3 * j + 1], dz = pz - pts[3 * j + 2];
    return __float_as_uint(dx * dx + dy * dy + dz * dz);
}

// queries in Morton order, one wave each; dist[idx[i]] = mean distance of sorted point i
__global__ __launch_bounds__(256) void sorg_knn_kernel(const float *__restrict__ pts, const int *__restrict__ idx,
                                                       const int *__restrict__ d_m, int mean_k,
                                                       const float *__restrict__ box1, const float *__restrict__ box2,
                                                       const float *__restrict__ box3, float *__restrict__ dist)
{
    __shared__ unsigned s_buf[KNN_WAVES][KNN_CAP];
    const int m = *d_m;
    const int lane = threadIdx.x & 63;
    const int i = __builtin_amdgcn_readfirstlane(blockIdx.x * KNN_WAVES + (threadIdx.x >> 6));
    if (i >= m)
        return;
    const int kk = mean_k < m - 1 ? mean_k : m - 1;
    if (kk <= 0) {
        if (lane == 0)
            dist[idx[i]] = 0.f;
        return;
    }
    const float px = pts[3 * i], py = pts[3 * i + 1], pz = pts[3 * i + 2];
    KnnWave w;
    w.buf = s_buf[threadIdx.x >> 6];
    w.nb = 0;
    w.full = false;
    w.r2 = 0xffffffffu;
    w.kk = kk;
    w.lane = lane;

    // seed: the query's neighbours in Morton order, at least kk other points (m - 1 >= kk)
    const int h = (kk + 1) / 2 + 32, span = 2 * h + 1;
    int w1 = min(m, max(i - h, 0) + span);
    const int w0 = max(0, w1 - span);
    for (int base = w0; base < w1; base += 64) {
        const int j = base + lane;
        const bool cand = j < w1 && j != i;
        knn_append(w, cand, cand ? dist2_bits(pts, j, px, py, pz) : 0u);
    }
    knn_cut(w);

    // the hierarchy, boxes skipped when provably too far (tested when a level's children are listed, and again with the
    // tighter bound of the moment before a box is entered); the seed window is not visited twice
    const int n1 = (m + 63) >> 6, n2 = (n1 + 63) >> 6, n3 = (n2 + 63) >> 6;  // n3 <= 16
    const double md3 = lane < n3 ? box_mind2(box3, lane, px, py, pz) : 0.0;
    for (unsigned long long m3 = __ballot(lane < n3 && !box_skippable(md3, w.r2)); m3; m3 &= m3 - 1) {
        const int k3 = __builtin_ctzll(m3);
        if (box_skippable(shfl_double(md3, k3), w.r2))
            continue;
        const int c2 = k3 * 64 + lane;
        const double md2 = c2 < n2 ? box_mind2(box2, c2, px, py, pz) : 0.0;
        for (unsigned long long m2 = __ballot(c2 < n2 && !box_skippable(md2, w.r2)); m2; m2 &= m2 - 1) {
            const int k2 = __builtin_ctzll(m2);
            if (w.nb >= kk + 64)
                knn_cut(w);
            if (box_skippable(shfl_double(md2, k2), w.r2))
                continue;
            const int c1 = (k3 * 64 + k2) * 64 + lane;
            const double md1 = c1 < n1 ? box_mind2(box1, c1, px, py, pz) : 0.0;
            for (unsigned long long m1 = __ballot(c1 < n1 && !box_skippable(md1, w.r2)); m1; m1 &= m1 - 1) {
                const int k1 = __builtin_ctzll(m1);
                if (w.nb >= kk + 64)
                    knn_cut(w);
                if (box_skippable(shfl_double(md1, k1), w.r2))
                    continue;
                const int j = ((k3 * 64 + k2) * 64 + k1) * 64 + lane;
                const bool cand = j < m && j != i && (j < w0 || j >= w1);
                knn_append(w, cand, cand ? dist2_bits(pts, j, px, py, pz) : 0u);
            }
        }
    }

    // the mean over the kk smallest (nb >= kk: every point not in the buffer was skipped only after a cut)
    const unsigned kth = knn_kth(w);
    int c_less = 0;
    double s_less = 0.;
    for (int t = lane; t < w.nb; t += 64) {
        const unsigned v = w.buf[t];
        if (v < kth) {
            c_less++;
            s_less += (double)sqrtf(__uint_as_float(v));
        }
    }
    c_less = svo::wave_sum_dpp(c_less);
    const double total = svo::wave_sum(s_less) + (double)(kk - c_less) * (double)sqrtf(__uint_as_float(kth));
    if (lane == 0)
        dist[idx[i]] = (float)(total / kk);
}


}  // namespace

// Device-pointer form, svo_launch_sor's contract for up to 2^22 points.  The outputs must not overlap the inputs.
int svo_launch_sor_large(svo_ctx *ctx, const float *xyz, const float *color, int cap, int mean_k, double stddev_mul,
                         float z_limit, float *xyz_out, float *color_out, int *d_count, float *d_mean_dist, int *d_pass)
{
    if (cap <= 0)
        return SVO_OK;
    if (cap > SVO_SOR_LARGE_MAX_N) {
        svo_set_error("svo_sor_filter_large: at most %d points per call", SVO_SOR_LARGE_MAX_N);
        return SVO_ERR_CAPACITY;
    }
    if (mean_k < 1 || mean_k > SVO_SOR_LARGE_MAX_K) {
        svo_set_error("svo_sor_filter_large: mean_k %d outside 1..%d", mean_k, SVO_SOR_LARGE_MAX_K);
        return SVO_ERR_ARG;
    }
    const size_t n = (size_t)cap;
    const int nb1 = (cap + 63) / 64, nb2 = (nb1 + 63) / 64, nb3 = (nb2 + 63) / 64;
    const int nblk = (cap + RS_TILE - 1) / RS_TILE;
    // layout of the work buffer
    size_t off = 0;
    const size_t o_k0 = off; off = align256(off + n * 8);
    const size_t o_k1 = off; off = align256(off + n * 8);
    const size_t o_v0 = off; off = align256(off + n * 4);
    const size_t o_v1 = off; off = align256(off + n * 4);
    const size_t o_pts = off; off = align256(off + n * 12);
    const size_t o_b1 = off; off = align256(off + (size_t)nb1 * 24);
    const size_t o_b2 = off; off = align256(off + (size_t)nb2 * 24);
    const size_t o_b3 = off; off = align256(off + (size_t)nb3 * 24);
    const size_t o_hist = off; off = align256(off + (size_t)256 * nblk * 4);
    const size_t o_bnd = off; off = align256(off + 64);
    int rc;
    if ((rc = ctx->sor_grid.ensure(off)) || (rc = ctx->w_a.ensure(n * 12)) || (rc = ctx->w_b.ensure(n * 12)) ||
        (rc = ctx->w_c.ensure(n * 4)) || (rc = ctx->w_d.ensure(n + 64)) || (rc = ctx->w_e.ensure(64)))
        return rc;
    char *g = ctx->sor_grid.as<char>();
    uint64_t *k0 = reinterpret_cast<uint64_t *>(g + o_k0), *k1 = reinterpret_cast<uint64_t *>(g + o_k1);
    int *v0 = reinterpret_cast<int *>(g + o_v0), *v1 = reinterpret_cast<int *>(g + o_v1);
    float *pts = reinterpret_cast<float *>(g + o_pts);
    float *b1 = reinterpret_cast<float *>(g + o_b1), *b2 = reinterpret_cast<float *>(g + o_b2),
          *b3 = reinterpret_cast<float *>(g + o_b3);
    unsigned *hist = reinterpret_cast<unsigned *>(g + o_hist);
    double *bnd = reinterpret_cast<double *>(g + o_bnd);
    float *xyz_c = ctx->w_a.as<float>(), *col_c = ctx->w_b.as<float>();
    float *dist = d_mean_dist ? d_mean_dist : ctx->w_c.as<float>();
    uint8_t *mask = ctx->w_d.as<uint8_t>();
    int *d_m = d_pass ? d_pass : ctx->w_e.as<int>();
    hipStream_t st = ctx->stream;
    const dim3 b256(256), g256((cap + 255) / 256);
    hipLaunchKernelGGL(sorg_zmask_kernel, g256, b256, 0, st, xyz, cap, z_limit, mask);
    if ((rc = svo_launch_compact(ctx, mask, cap, nullptr, xyz, 3, xyz_c, color, color ? 3 : 0, color ? col_c : nullptr,
                                 nullptr, 0, nullptr, d_m)))
        return rc;
    hipLaunchKernelGGL(sorg_bounds_kernel, dim3(1), dim3(1024), 0, st, xyz_c, d_m, bnd);
    hipLaunchKernelGGL(sorg_key_kernel, g256, b256, 0, st, xyz_c, d_m, bnd, cap, k0, v0);
    if ((rc = radix_sort_pairs(st, k0, v0, k1, v1, cap, hist)))
        return rc;
    hipLaunchKernelGGL(sorg_gather_kernel, g256, b256, 0, st, xyz_c, v0, d_m, cap, pts);
    hipLaunchKernelGGL(sorg_box_kernel, dim3((nb1 + 3) / 4), b256, 0, st, pts, d_m, 1, nb1, b1);
    hipLaunchKernelGGL(sorg_box_kernel, dim3((nb2 + 3) / 4), b256, 0, st, b1, d_m, 2, nb2, b2);
    hipLaunchKernelGGL(sorg_box_kernel, dim3((nb3 + 3) / 4), b256, 0, st, b2, d_m, 3, nb3, b3);
    hipLaunchKernelGGL(sorg_knn_kernel, dim3((cap + KNN_WAVES - 1) / KNN_WAVES), dim3(64 * KNN_WAVES), 0, st, pts, v0,
                       d_m, mean_k, b1, b2, b3, dist);
    hipLaunchKernelGGL(sor_threshold_kernel, dim3(1), dim3(1024), 0, st, dist, d_m, stddev_mul, cap, mask);
    if ((rc = svo_launch_compact(ctx, mask, cap, d_m, xyz_c, 3, xyz_out, color ? col_c : nullptr, color ? 3 : 0,
                                 color ? color_out : nullptr, nullptr, 0, nullptr, d_count)))
        return rc;
    SVO_HIP(hipGetLastError());
    return SVO_OK;
}

extern "C" int svo_sor_filter_large(svo_ctx *ctx, const float *xyz, const float *color, int n, int mean_k,
                                    double stddev_mul, float z_limit, float *xyz_out, float *color_out, int *n_out,
                                    float *mean_dist_out, int *n_pass_out, int mem)
{
    SVO_CHECK_ARG(ctx && n >= 0 && mean_k > 0 && mean_k <= SVO_SOR_LARGE_MAX_K && n_out);
    SVO_CHECK_ARG(mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE);
    *n_out = 0;
    if (n_pass_out)
        *n_pass_out = 0;
    if (n > SVO_SOR_LARGE_MAX_N) {
        svo_set_error("svo_sor_filter_large: %d points, at most %d per call", n, SVO_SOR_LARGE_MAX_N);
        return SVO_ERR_CAPACITY;
    }
    if (n == 0)
        return SVO_OK;
    SVO_CHECK_ARG(xyz && xyz_out && (!color || color_out));
    int rc;
    if ((rc = ctx->s_g.ensure(64)))
        return rc;
    int *d_cnt = ctx->s_g.as<int>();  // [0] kept, [1] passed the pre-filter
    const float *dx = xyz, *dc = color;
    float *ox = xyz_out, *oc = color_out, *od = mean_dist_out;
    if (mem == SVO_MEM_HOST) {
        if ((rc = ctx->s_a.ensure((size_t)n * 12)) || (rc = ctx->s_b.ensure((size_t)n * 12)) ||
            (rc = ctx->s_c.ensure((size_t)n * 12)) || (rc = ctx->s_d.ensure((size_t)n * 12)) ||
            (rc = ctx->s_e.ensure((size_t)n * 4)))
            return rc;
        SVO_HIP(hipMemcpyAsync(ctx->s_a.p, xyz, (size_t)n * 12, hipMemcpyHostToDevice, ctx->stream));
        if (color)
            SVO_HIP(hipMemcpyAsync(ctx->s_b.p, color, (size_t)n * 12, hipMemcpyHostToDevice, ctx->stream));
        dx = ctx->s_a.as<float>();
        dc = color ? ctx->s_b.as<float>() : nullptr;
        ox = ctx->s_c.as<float>();
        oc = ctx->s_d.as<float>();
        od = ctx->s_e.as<float>();
    }
    if ((rc = svo_launch_sor_large(ctx, dx, dc, n, mean_k, stddev_mul, z_limit, ox, oc, d_cnt, od, d_cnt + 1)))
        return rc;
    SVO_HIP(hipMemcpyAsync(ctx->pinned, d_cnt, 8, hipMemcpyDeviceToHost, ctx->stream));
    SVO_HIP(hipStreamSynchronize(ctx->stream));
    const int kept = reinterpret_cast<int *>(ctx->pinned)[0], passed = reinterpret_cast<int *>(ctx->pinned)[1];
    *n_out = kept;
    if (n_pass_out)
        *n_pass_out = passed;
    if (mem == SVO_MEM_HOST) {
        if (kept > 0) {
            SVO_HIP(hipMemcpyAsync(xyz_out, ox, (size_t)kept * 12, hipMemcpyDeviceToHost, ctx->stream));
            if (color)
                SVO_HIP(hipMemcpyAsync(color_out, oc, (size_t)kept * 12, hipMemcpyDeviceToHost, ctx->stream));
        }
        if (mean_dist_out && passed > 0)
            SVO_HIP(hipMemcpyAsync(mean_dist_out, od, (size_t)passed * 4, hipMemcpyDeviceToHost, ctx->stream));
        SVO_HIP(hipStreamSynchronize(ctx->stream));
    }
    return SVO_OK;
}
