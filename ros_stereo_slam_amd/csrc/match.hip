// match.hip -- brute-force descriptor matching: cv::BFMatcher(normType, false).knnMatch and the ratio-test loop the
// reference runs after it (src/triangulation.cpp:123-133; the same block at src/StereoCV.cpp:77-88,136-147,
// src/bundleAdjust.cpp:269-271, include/trangulation.h:51-53).
//
// svo_knn_match: an all-pairs search with a running top-4 per query.  A lane owns one query; the train rows go through
// LDS in tiles of MT rows that every lane of the workgroup reads as broadcasts; a lane keeps MT accumulators, walks the
// row four 32-bit words at a time (its own query words come straight from memory: every word is read once per tile and
// used MT times) and then offers the MT keys to its sorted list of (key << 32 | train index) entries.  One 64-bit
// compare orders by key first and by train index on equal keys, so ties go to the lower index wherever they meet.  With
// few queries the train range is split over workgroups (blockIdx.y); knn_merge_kernel merges the partial lists with the
// same compare and writes idx / dist.  No distance matrix exists anywhere: 32 bytes per query and split is all that
// reaches HBM.
//
// The float key is the stated sum -- t = a_i - b_i, s = s + t * t, one accumulator per pair, index order, no FMA (the
// library is built with -ffp-contract=off) -- and rows are padded with zero words, which add +0 to a sum that is never
// negative: the padding cannot change a bit.  The inner loops: the float norm a subtraction, a multiplication and an
// addition per pair element (packed two at a time) and one LDS broadcast per four elements; the byte norm one
// v_dot4_u32_u8 per four elements; the binary norm an xor and a popcount-add per word.  Measured times and what bounds
// them: DESIGN.md section 10c.
#include <cmath>

#include "svo_internal.h"

namespace {

constexpr int MT = 32;          // train rows per LDS tile = accumulators per lane
constexpr int MQ = 256;         // queries per workgroup, one per lane
constexpr int MAX_ROWS = 32768; // queries / train rows per problem
constexpr int MAX_SPLIT = 64;   // workgroups one query's train range is split over at most
constexpr int TARGET_GROUPS = 1024;
constexpr unsigned long long EMPTY = ~0ull;  // idx -1, behind every key

struct MatchProb {
    int q0, nq, t0, nt;
};
struct MatchBatch {
    MatchProb p[SVO_LK_MAX_JOBS];
};

// sorted insertion; entries are unique (the train index is part of them), so strict compares suffice
__device__ __forceinline__ void offer(unsigned long long (&best)[4], unsigned long long e)
{
    if (e < best[3]) {
        best[3] = e;
#pragma unroll
        for (int s = 3; s > 0; s--)
            if (best[s] < best[s - 1]) {
                const unsigned long long t = best[s];
                best[s] = best[s - 1];
                best[s - 1] = t;
            }
    }
}

__device__ __forceinline__ unsigned dot4(unsigned a, unsigned b, unsigned c)
{
#if __has_builtin(__builtin_amdgcn_udot4)
    return __builtin_amdgcn_udot4(a, b, c, false);
#else
    return c + (a & 255u) * (b & 255u) + ((a >> 8) & 255u) * ((b >> 8) & 255u) + ((a >> 16) & 255u) * ((b >> 16) & 255u) +
           (a >> 24) * (b >> 24);
#endif
}

template <int NORM> __device__ __forceinline__ void step(unsigned q, unsigned t, float &sf, unsigned &si)
{
    if (NORM == SVO_MATCH_L2_F32) {
        const float d = __uint_as_float(q) - __uint_as_float(t);
        sf = sf + d * d;
    } else if (NORM == SVO_MATCH_L2_U8) {
        si = dot4(q, t, si);
    } else {
        si += __popc(q ^ t);
    }
}

// grid: (query blocks, splits, problems).  Q / T: rows of W words.  vec: the query rows may be read 16 bytes at a time.
// part: per query row and split four entries, best first.
template <int NORM>
__global__ __launch_bounds__(MQ) void knn_partial_kernel(MatchBatch b, const uint32_t *__restrict__ Q,
                                                         const uint32_t *__restrict__ T, int W, int vec, int nsplit,
                                                         unsigned long long *__restrict__ part)
{
    const MatchProb pr = b.p[blockIdx.z];
    const int qb = blockIdx.x * MQ;
    if (qb >= pr.nq)
        return;
    extern __shared__ __align__(16) uint32_t sm[];  // MT rows of WP words, then MT squared norms (bytes)
    const int WP = (W + 3) & ~3;
    uint32_t *sm_norm = sm + MT * WP;
    const int ntiles = (pr.nt + MT - 1) / MT;
    const int per = (ntiles + nsplit - 1) / nsplit;
    const int tile0 = blockIdx.y * per;
    const int tile1 = tile0 + per < ntiles ? tile0 + per : ntiles;
    const int lq = qb + threadIdx.x;
    const bool live = lq < pr.nq;
    const uint32_t *qrow = Q + (size_t)(pr.q0 + (live ? lq : pr.nq - 1)) * W;
    unsigned long long best[4] = {EMPTY, EMPTY, EMPTY, EMPTY};
    unsigned qn = 0;
    if (NORM == SVO_MATCH_L2_U8)
        for (int d = 0; d < W; d++)
            qn = dot4(qrow[d], qrow[d], qn);
    for (int tile = tile0; tile < tile1; tile++) {
        const int r0 = tile * MT;
        const int rows = pr.nt - r0 < MT ? pr.nt - r0 : MT;
        const uint32_t *trow = T + (size_t)(pr.t0 + r0) * W;
        __syncthreads();  // the previous tile has been read
        for (int e = threadIdx.x; e < MT * WP; e += MQ) {
            const int r = e / WP, c = e - r * WP;
            sm[e] = (r < rows && c < W) ? trow[(size_t)r * W + c] : 0u;
        }
        if (NORM == SVO_MATCH_L2_U8 && threadIdx.x < MT) {
            unsigned tn = 0;
            if ((int)threadIdx.x < rows)
                for (int d = 0; d < W; d++) {
                    const unsigned w = trow[(size_t)threadIdx.x * W + d];
                    tn = dot4(w, w, tn);
                }
            sm_norm[threadIdx.x] = tn;
        }
        __syncthreads();
        float sf[MT];
        unsigned si[MT];
#pragma unroll
        for (int j = 0; j < MT; j++)
            sf[j] = 0.f, si[j] = 0u;
        for (int d0 = 0; d0 < WP; d0 += 4) {
            uint4 q4;
            if (vec) {
                q4 = *reinterpret_cast<const uint4 *>(qrow + d0);
            } else {
                q4.x = qrow[d0];  // d0 < W always
                q4.y = d0 + 1 < W ? qrow[d0 + 1] : 0u;
                q4.z = d0 + 2 < W ? qrow[d0 + 2] : 0u;
                q4.w = d0 + 3 < W ? qrow[d0 + 3] : 0u;
            }
#pragma unroll
            for (int j = 0; j < MT; j++) {
                const uint4 t4 = *reinterpret_cast<const uint4 *>(sm + j * WP + d0);
                step<NORM>(q4.x, t4.x, sf[j], si[j]);
                step<NORM>(q4.y, t4.y, sf[j], si[j]);
                step<NORM>(q4.z, t4.z, sf[j], si[j]);
                step<NORM>(q4.w, t4.w, sf[j], si[j]);
            }
        }
#pragma unroll
        for (int j = 0; j < MT; j++)
            if (j < rows) {
                unsigned key;
                if (NORM == SVO_MATCH_L2_F32)
                    key = sf[j] != sf[j] ? 0x7fc00000u : __float_as_uint(sf[j]);  // a NaN sorts behind +inf
                else if (NORM == SVO_MATCH_L2_U8)
                    key = qn + sm_norm[j] - 2u * si[j];
                else
                    key = si[j];
                // after the first tiles a new entry is rare: the wave skips the insertion unless a lane has one
                const unsigned long long e = ((unsigned long long)key << 32) | (unsigned)(r0 + j);
                if (__any(e < best[3]))
                    offer(best, e);
            }
    }
    if (live) {
        unsigned long long *o = part + ((size_t)(pr.q0 + lq) * nsplit + blockIdx.y) * 4;
#pragma unroll
        for (int s = 0; s < 4; s++)
            o[s] = best[s];
    }
}

// grid: (query blocks, problems); a lane merges the nsplit lists of its query and writes its k slots
__global__ __launch_bounds__(256) void knn_merge_kernel(MatchBatch b, const unsigned long long *__restrict__ part, int nsplit,
                                                        int k, int norm, int *__restrict__ idx, float *__restrict__ dist)
{
    const MatchProb pr = b.p[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= pr.nq)
        return;
    const size_t row = (size_t)pr.q0 + i;
    unsigned long long best[4] = {EMPTY, EMPTY, EMPTY, EMPTY};
    const unsigned long long *in = part + row * nsplit * 4;
    for (int e = 0; e < nsplit * 4; e++)
        offer(best, in[e]);
    for (int s = 0; s < k; s++) {
        const unsigned long long e = best[s];
        const unsigned key = (unsigned)(e >> 32);
        int id = -1;
        float d = INFINITY;
        if (e != EMPTY) {
            id = (int)(unsigned)e;
            // the double root of a float (or of an integer below 2^24) rounded to float is the correctly rounded
            // float root: 53 >= 2 * 24 + 2
            if (norm == SVO_MATCH_L2_F32)
                d = (float)sqrt((double)__uint_as_float(key));
            else if (norm == SVO_MATCH_L2_U8)
                d = (float)sqrt((double)key);
            else
                d = (float)key;
        }
        idx[row * k + s] = id;
        dist[row * k + s] = d;
    }
}

// the test of src/triangulation.cpp:129 per query, and the train point it would pair with
__global__ void ratio_mask_kernel(const int *__restrict__ idx, const float *__restrict__ dist, int nq, int k, double ratio,
                                  const float2 *__restrict__ xy_train, uint8_t *__restrict__ mask, float2 *__restrict__ pick)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq)
        return;
    bool keep = false;
    if (k >= 2 && idx[(size_t)i * k + 1] >= 0 && idx[(size_t)i * k] >= 0) {
        const double rhs = ratio * (double)dist[(size_t)i * k + 1];
        keep = (double)dist[(size_t)i * k] < rhs;
    }
    mask[i] = keep ? 1 : 0;
    pick[i] = keep ? xy_train[idx[(size_t)i * k]] : make_float2(0.f, 0.f);
}

int check_offsets(const int *off, int nprob, int *lo, int *hi, bool *too_big)
{
    SVO_CHECK_ARG(off && off[0] >= 0);
    for (int p = 0; p < nprob; p++) {
        SVO_CHECK_ARG(off[p + 1] >= off[p]);
        if (off[p + 1] - off[p] > MAX_ROWS)
            *too_big = true;
    }
    *lo = off[0];
    *hi = off[nprob];
    return SVO_OK;
}

}  // namespace

extern "C" int svo_knn_match(svo_ctx *ctx, int norm, const void *query, const void *train, int dim, const int *q_offsets,
                             const int *t_offsets, int nprob, int k, int *idx, float *dist, int mem)
{
    SVO_CHECK_ARG(ctx && (mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE));
    SVO_CHECK_ARG(norm == SVO_MATCH_L2_F32 || norm == SVO_MATCH_L2_U8 || norm == SVO_MATCH_HAMMING);
    SVO_CHECK_ARG(k >= 1 && k <= 4 && nprob >= 1 && nprob <= SVO_LK_MAX_JOBS);
    if (norm == SVO_MATCH_L2_F32)
        SVO_CHECK_ARG(dim >= 1 && dim <= 256);
    else if (norm == SVO_MATCH_L2_U8)
        SVO_CHECK_ARG(dim >= 4 && dim <= 256 && dim % 4 == 0);
    else
        SVO_CHECK_ARG(dim >= 1 && dim <= 16);
    const int W = norm == SVO_MATCH_L2_U8 ? dim / 4 : dim;  // 32-bit words per row
    int rc, qlo = 0, qhi = 0, tlo = 0, thi = 0;
    bool too_big = false;
    if ((rc = check_offsets(q_offsets, nprob, &qlo, &qhi, &too_big)) || (rc = check_offsets(t_offsets, nprob, &tlo, &thi, &too_big)))
        return rc;
    SVO_CHECK_ARG(qhi == qlo || (query && idx && dist));
    SVO_CHECK_ARG(thi == tlo || train);
    SVO_CHECK_ARG((reinterpret_cast<uintptr_t>(query) & 3) == 0 && (reinterpret_cast<uintptr_t>(train) & 3) == 0);
    if (too_big) {
        svo_set_error("svo_knn_match: at most %d queries and %d train rows per problem", MAX_ROWS, MAX_ROWS);
        return SVO_ERR_CAPACITY;
    }
    if (qhi == qlo)
        return SVO_OK;  // no query anywhere: nothing is written
    MatchBatch b;
    int qblocks = 0, qblocks_max = 0, tiles_max = 0, nq_max = 0;
    for (int p = 0; p < SVO_LK_MAX_JOBS; p++) {
        const int s = p < nprob ? p : 0;
        b.p[p] = MatchProb{q_offsets[s], q_offsets[s + 1] - q_offsets[s], t_offsets[s], t_offsets[s + 1] - t_offsets[s]};
        if (p >= nprob)
            continue;
        const int qb = (b.p[p].nq + MQ - 1) / MQ, tl = (b.p[p].nt + MT - 1) / MT;
        qblocks += qb;
        qblocks_max = qb > qblocks_max ? qb : qblocks_max;
        tiles_max = tl > tiles_max ? tl : tiles_max;
        nq_max = b.p[p].nq > nq_max ? b.p[p].nq : nq_max;
    }
    int nsplit = (TARGET_GROUPS + qblocks - 1) / qblocks;
    nsplit = nsplit > MAX_SPLIT ? MAX_SPLIT : nsplit;
    nsplit = nsplit > tiles_max ? tiles_max : nsplit;
    nsplit = nsplit < 1 ? 1 : nsplit;
    const size_t row_b = (size_t)W * 4;
    if ((rc = ctx->w_a.ensure((size_t)qhi * nsplit * 4 * sizeof(unsigned long long))))
        return rc;
    const uint32_t *dq = static_cast<const uint32_t *>(query), *dt = static_cast<const uint32_t *>(train);
    int *didx = idx;
    float *ddist = dist;
    if (mem == SVO_MEM_HOST) {
        if ((rc = ctx->s_a.ensure((size_t)qhi * row_b)) || (rc = ctx->s_b.ensure((size_t)(thi > 0 ? thi : 1) * row_b)) ||
            (rc = ctx->s_c.ensure((size_t)qhi * k * 4)) || (rc = ctx->s_d.ensure((size_t)qhi * k * 4)))
            return rc;
        SVO_HIP(hipMemcpyAsync(ctx->s_a.as<char>() + (size_t)qlo * row_b, static_cast<const char *>(query) + (size_t)qlo * row_b,
                               (size_t)(qhi - qlo) * row_b, hipMemcpyHostToDevice, ctx->stream));
        if (thi > tlo)
            SVO_HIP(hipMemcpyAsync(ctx->s_b.as<char>() + (size_t)tlo * row_b, static_cast<const char *>(train) + (size_t)tlo * row_b,
                                   (size_t)(thi - tlo) * row_b, hipMemcpyHostToDevice, ctx->stream));
        dq = ctx->s_a.as<uint32_t>();
        dt = ctx->s_b.as<uint32_t>();
        didx = ctx->s_c.as<int>();
        ddist = ctx->s_d.as<float>();
    }
    const int vec = (W % 4 == 0 && (reinterpret_cast<uintptr_t>(dq) & 15) == 0) ? 1 : 0;
    const int WP = (W + 3) & ~3;
    const size_t lds = (size_t)(MT * WP + MT) * sizeof(uint32_t);
    unsigned long long *part = ctx->w_a.as<unsigned long long>();
    const dim3 grid(qblocks_max, nsplit, nprob), block(MQ);
    if (norm == SVO_MATCH_L2_F32)
        hipLaunchKernelGGL(knn_partial_kernel<SVO_MATCH_L2_F32>, grid, block, lds, ctx->stream, b, dq, dt, W, vec, nsplit, part);
    else if (norm == SVO_MATCH_L2_U8)
        hipLaunchKernelGGL(knn_partial_kernel<SVO_MATCH_L2_U8>, grid, block, lds, ctx->stream, b, dq, dt, W, vec, nsplit, part);
    else
        hipLaunchKernelGGL(knn_partial_kernel<SVO_MATCH_HAMMING>, grid, block, lds, ctx->stream, b, dq, dt, W, vec, nsplit, part);
    hipLaunchKernelGGL(knn_merge_kernel, dim3((nq_max + 255) / 256, nprob), dim3(256), 0, ctx->stream, b, part, nsplit, k, norm,
                       didx, ddist);
    SVO_HIP(hipGetLastError());
    if (mem == SVO_MEM_DEVICE)
        return SVO_OK;
    const size_t o = (size_t)qlo * k, n = (size_t)(qhi - qlo) * k * 4;
    SVO_HIP(hipMemcpyAsync(idx + o, didx + o, n, hipMemcpyDeviceToHost, ctx->stream));
    SVO_HIP(hipMemcpyAsync(dist + o, ddist + o, n, hipMemcpyDeviceToHost, ctx->stream));
    SVO_HIP(hipStreamSynchronize(ctx->stream));
    return SVO_OK;
}

extern "C" int svo_ratio_pairs(svo_ctx *ctx, const int *idx, const float *dist, int nq, int k, double ratio,
                               const float *xy_query, const float *xy_train, float *p1, float *p2, uint8_t *mask, int *count,
                               int mem)
{
    SVO_CHECK_ARG(ctx && (mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE));
    SVO_CHECK_ARG(nq >= 0 && nq <= MAX_ROWS && k >= 1 && k <= 4 && count && !std::isnan(ratio));
    *count = 0;
    if (nq == 0)
        return SVO_OK;
    SVO_CHECK_ARG(idx && dist && xy_query && xy_train && p1 && p2);
    int rc;
    if ((rc = ctx->w_a.ensure((size_t)nq * 8)) || (rc = ctx->w_b.ensure((size_t)nq)) || (rc = ctx->w_c.ensure(64)))
        return rc;
    const int *didx = idx;
    const float *ddist = dist, *dxq = xy_query, *dxt = xy_train;
    float *d1 = p1, *d2 = p2;
    uint8_t *dmask = mask ? mask : ctx->w_b.as<uint8_t>();
    if (mem == SVO_MEM_HOST) {
        int nt = 1;  // train points the pairs can name
        for (int i = 0; i < nq; i++)
            nt = idx[(size_t)i * k] + 1 > nt ? idx[(size_t)i * k] + 1 : nt;
        const size_t kb = (size_t)nq * k * 4;
        if ((rc = ctx->s_a.ensure(kb)) || (rc = ctx->s_b.ensure(kb)) || (rc = ctx->s_c.ensure((size_t)nq * 8)) ||
            (rc = ctx->s_d.ensure((size_t)nt * 8)) || (rc = ctx->s_e.ensure((size_t)nq * 8)) ||
            (rc = ctx->s_f.ensure((size_t)nq * 8)))
            return rc;
        SVO_HIP(hipMemcpyAsync(ctx->s_a.p, idx, kb, hipMemcpyHostToDevice, ctx->stream));
        SVO_HIP(hipMemcpyAsync(ctx->s_b.p, dist, kb, hipMemcpyHostToDevice, ctx->stream));
        SVO_HIP(hipMemcpyAsync(ctx->s_c.p, xy_query, (size_t)nq * 8, hipMemcpyHostToDevice, ctx->stream));
        SVO_HIP(hipMemcpyAsync(ctx->s_d.p, xy_train, (size_t)nt * 8, hipMemcpyHostToDevice, ctx->stream));
        didx = ctx->s_a.as<int>();
        ddist = ctx->s_b.as<float>();
        dxq = ctx->s_c.as<float>();
        dxt = ctx->s_d.as<float>();
        d1 = ctx->s_e.as<float>();
        d2 = ctx->s_f.as<float>();
        dmask = ctx->w_b.as<uint8_t>();
    }
    float *pick = ctx->w_a.as<float>();
    int *dcount = ctx->w_c.as<int>();
    hipLaunchKernelGGL(ratio_mask_kernel, dim3((nq + 255) / 256), dim3(256), 0, ctx->stream, didx, ddist, nq, k, ratio,
                       reinterpret_cast<const float2 *>(dxt), dmask, reinterpret_cast<float2 *>(pick));
    if ((rc = svo_launch_compact(ctx, dmask, nq, nullptr, dxq, 2, d1, pick, 2, d2, nullptr, 0, nullptr, dcount)))
        return rc;
    SVO_HIP(hipMemcpyAsync(ctx->pinned, dcount, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    SVO_HIP(hipStreamSynchronize(ctx->stream));
    const int kept = *reinterpret_cast<int *>(ctx->pinned);
    *count = kept;
    if (mem == SVO_MEM_HOST) {
        if (kept > 0) {
            SVO_HIP(hipMemcpyAsync(p1, d1, (size_t)kept * 8, hipMemcpyDeviceToHost, ctx->stream));
            SVO_HIP(hipMemcpyAsync(p2, d2, (size_t)kept * 8, hipMemcpyDeviceToHost, ctx->stream));
        }
        if (mask)
            SVO_HIP(hipMemcpyAsync(mask, dmask, (size_t)nq, hipMemcpyDeviceToHost, ctx->stream));
        SVO_HIP(hipStreamSynchronize(ctx->stream));
    }
    return SVO_OK;
}
