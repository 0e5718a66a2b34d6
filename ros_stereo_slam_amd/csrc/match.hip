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
//
// The same tile loop serves the rest of cv::BFMatcher (host arithmetic: match_plan.hip.h):
//   svo_knn_match_gated  SEARCH_MASK / SEARCH_GATE: a lane forms the 32 candidate bits of its query for the tile -- bytes of the
//                        mask, or the epipolar band from the key points (the tile's train points sit in LDS) -- and a wave none
//                        of whose lanes has a candidate leaves the tile after that test; a pair that is no candidate is offered
//                        as EMPTY, which no list takes.
//   svo_match_cross      the search above with the roles swapped (every train row's best query); cross_cv_kernel lets each
//                        train row bid for its query with a 64-bit atomicMin of (key << 32 | train row) and cross_finish_kernel
//                        writes the winners; cross_mutual_kernel looks a query's best train row up in the reverse lists.
//   svo_radius_match     SEARCH_COUNT counts the keys up to the radius' largest key per query and split, radius_scan_kernel
//                        turns the counts into positions (the block scan of scan_ops.hip.h), SEARCH_WRITE stores
//                        (key << 32 | train row) entries there and radius_sort_kernel sorts one query's entries in LDS and
//                        writes idx / dist.
#include <cmath>

#include "match_plan.hip.h"
#include "scan_ops.hip.h"
#include "svo_internal.h"

namespace {

using match_plan::MAX_ROWS;
using match_plan::MAX_SPLIT;
using match_plan::MQ;
using match_plan::MT;
using match_plan::TARGET_GROUPS;
static_assert(match_plan::MAX_PROB == SVO_LK_MAX_JOBS, "one batch size");
constexpr unsigned long long EMPTY = ~0ull;  // idx -1, behind every key
constexpr unsigned NAN_KEY = 0x7fc00000u;    // the float norm's key of a NaN sum: behind +inf

struct MatchProb {
    int q0, nq, t0, nt;
};
struct MatchBatch {
    MatchProb p[SVO_LK_MAX_JOBS];
};

enum { SEARCH_KNN = 0, SEARCH_MASK = 1, SEARCH_GATE = 2, SEARCH_COUNT = 3, SEARCH_WRITE = 4 };
// what the modes other than SEARCH_KNN read
struct SearchExtra {
    const uint8_t *mask;                        // SEARCH_MASK: problem p's matrix at mask + mask_off[p]
    unsigned long long mask_off[SVO_LK_MAX_JOBS];
    const float2 *xy_query, *xy_train;          // SEARCH_GATE: a point per row of Q / T
    float dy_max, dx_min, dx_max;
    long long key_max;                          // SEARCH_COUNT / SEARCH_WRITE: the largest key that passes, -1 = none
    int *counts;                                // per query row and split: matches (COUNT), then their start within the row (WRITE)
    const int *row_start;                       // SEARCH_WRITE: where a query row's matches start
    const int *scal;                            // SEARCH_WRITE: [total, longest row, fits]
    unsigned long long *entries;
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
// part: per query row and split four entries, best first (the SEARCH_KNN / MASK / GATE modes).
template <int NORM, int MODE>
__global__ __launch_bounds__(MQ) void knn_partial_kernel(MatchBatch b, const uint32_t *__restrict__ Q,
                                                         const uint32_t *__restrict__ T, int W, int vec, int nsplit,
                                                         unsigned long long *__restrict__ part, SearchExtra x)
{
    const MatchProb pr = b.p[blockIdx.z];
    const int qb = blockIdx.x * MQ;
    if (qb >= pr.nq)
        return;
    if (MODE == SEARCH_WRITE && x.scal[2] == 0)
        return;  // the matches do not fit: nothing is written
    extern __shared__ __align__(16) uint32_t sm[];  // MT rows of WP words, then MT squared norms (bytes), then MT train points
    const int WP = (W + 3) & ~3;
    uint32_t *sm_norm = sm + MT * WP;
    float2 *sm_xy = reinterpret_cast<float2 *>(sm_norm + MT);
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
    float2 qxy = make_float2(0.f, 0.f);
    if (MODE == SEARCH_GATE && live)
        qxy = x.xy_query[pr.q0 + lq];
    int found = 0, at = 0;  // SEARCH_COUNT: matches so far; SEARCH_WRITE: the next entry of this query and split
    if (MODE == SEARCH_WRITE && live)
        at = x.row_start[pr.q0 + lq] + x.counts[(size_t)(pr.q0 + lq) * nsplit + blockIdx.y];
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
        if (MODE == SEARCH_GATE && threadIdx.x < MT)
            sm_xy[threadIdx.x] = (int)threadIdx.x < rows ? x.xy_train[pr.t0 + r0 + threadIdx.x] : make_float2(0.f, 0.f);
        __syncthreads();
        // the candidates of this lane's query among the tile's rows, one bit each; a wave without any leaves the tile here
        // (wave-uniform, and behind the barrier: the next tile's barriers are met by every wave all the same)
        unsigned cand = ~0u;
        if (MODE == SEARCH_MASK) {
            cand = 0u;
            if (live) {
                const uint8_t *m = x.mask + x.mask_off[blockIdx.z] + (size_t)lq * pr.nt + r0;
                for (int j = 0; j < rows; j++)
                    cand |= m[j] ? 1u << j : 0u;
            }
        }
        if (MODE == SEARCH_GATE) {
            cand = 0u;
            if (live)
                for (int j = 0; j < rows; j++) {
                    const float2 t = sm_xy[j];
                    const float dy = qxy.y - t.y, ady = fabsf(dy), dx = qxy.x - t.x;
                    cand |= (ady <= x.dy_max && dx >= x.dx_min && dx <= x.dx_max) ? 1u << j : 0u;
                }
        }
        if ((MODE == SEARCH_MASK || MODE == SEARCH_GATE) && !__any(cand != 0u))
            continue;
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
                unsigned long long e = ((unsigned long long)key << 32) | (unsigned)(r0 + j);
                if (MODE == SEARCH_COUNT || MODE == SEARCH_WRITE) {
                    const bool pass = live && (long long)key <= x.key_max;
                    if (MODE == SEARCH_COUNT)
                        found += pass ? 1 : 0;
                    else if (pass)
                        x.entries[at++] = e;
                    continue;
                }
                if ((MODE == SEARCH_MASK || MODE == SEARCH_GATE) && !((cand >> j) & 1u))
                    e = EMPTY;
                if (__any(e < best[3]))
                    offer(best, e);
            }
    }
    if (MODE == SEARCH_COUNT) {
        if (live)
            x.counts[(size_t)(pr.q0 + lq) * nsplit + blockIdx.y] = found;
        return;
    }
    if (MODE == SEARCH_WRITE)
        return;
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

// dist of a key: knn_merge_kernel's arithmetic
__device__ __forceinline__ float dist_of(int norm, unsigned key)
{
    if (norm == SVO_MATCH_L2_F32)
        return (float)sqrt((double)__uint_as_float(key));
    if (norm == SVO_MATCH_L2_U8)
        return (float)sqrt((double)key);
    return (float)key;
}

// the best entry of a row's nsplit partial lists: each list is sorted, so the least of their heads
__device__ __forceinline__ unsigned long long best_of(const unsigned long long *__restrict__ part, size_t row, int nsplit)
{
    unsigned long long m = EMPTY;
    for (int s = 0; s < nsplit; s++) {
        const unsigned long long e = part[(row * nsplit + s) * 4];
        m = e < m ? e : m;
    }
    return m;
}

// SVO_CROSS_CV, the bids.  b: the REVERSE search (its query rows are the train rows).  grid: (train blocks, problems).  A train
// row bids (key << 32 | train row) for its best query; the least bid per query stands -- the smallest key, the lower train row
// on equal keys, whatever the order the bids arrive in.  A NaN key bids for nobody.  slot: EMPTY before the launch.
__global__ __launch_bounds__(256) void cross_cv_kernel(MatchBatch b, const unsigned long long *__restrict__ part, int nsplit,
                                                       unsigned long long *__restrict__ slot)
{
    const MatchProb pr = b.p[blockIdx.y];
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= pr.nq)
        return;
    const unsigned long long e = best_of(part, (size_t)pr.q0 + t, nsplit);
    if (e == EMPTY || (unsigned)(e >> 32) == NAN_KEY)  // only the float norm has a key this large
        return;
    atomicMin(&slot[(size_t)pr.t0 + (unsigned)e], (e & 0xffffffff00000000ull) | (unsigned)t);
}

// one (key << 32 | train row) entry, or EMPTY, per query row -> idx / dist.  b: the forward problems
__global__ __launch_bounds__(256) void cross_finish_kernel(MatchBatch b, const unsigned long long *__restrict__ slot, int norm,
                                                           int *__restrict__ idx, float *__restrict__ dist)
{
    const MatchProb pr = b.p[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= pr.nq)
        return;
    const unsigned long long e = slot[(size_t)pr.q0 + i];
    idx[(size_t)pr.q0 + i] = e == EMPTY ? -1 : (int)(unsigned)e;
    dist[(size_t)pr.q0 + i] = e == EMPTY ? INFINITY : dist_of(norm, (unsigned)(e >> 32));
}

// SVO_CROSS_MUTUAL.  b: the forward problems, fwd: their partial lists (nsf splits); rev: the reverse search's lists per train
// row (nsr splits).  Query i keeps its best train row j when j's best query is i.
__global__ __launch_bounds__(256) void cross_mutual_kernel(MatchBatch b, const unsigned long long *__restrict__ fwd, int nsf,
                                                           const unsigned long long *__restrict__ rev, int nsr, int norm,
                                                           int *__restrict__ idx, float *__restrict__ dist)
{
    const MatchProb pr = b.p[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= pr.nq)
        return;
    unsigned long long e = best_of(fwd, (size_t)pr.q0 + i, nsf);
    if (e != EMPTY) {
        const unsigned long long r = best_of(rev, (size_t)pr.t0 + (unsigned)e, nsr);
        if (r == EMPTY || (int)(unsigned)r != i)
            e = EMPTY;
    }
    idx[(size_t)pr.q0 + i] = e == EMPTY ? -1 : (int)(unsigned)e;
    dist[(size_t)pr.q0 + i] = e == EMPTY ? INFINITY : dist_of(norm, (unsigned)(e >> 32));
}

// a query without any train row, or a call without any: -1 / +inf
__global__ void cross_none_kernel(int lo, int hi, int *__restrict__ idx, float *__restrict__ dist)
{
    const int i = lo + blockIdx.x * blockDim.x + threadIdx.x;
    if (i < hi) {
        idx[i] = -1;
        dist[i] = INFINITY;
    }
}

// svo_radius_match, between its two passes: ONE workgroup.  counts[row * nsplit + s] (matches of a query row in split s) become
// their exclusive sums within the row; row_start[row] the sum of all rows before it (row_start[hi]: the total), the same numbers
// go to the caller's row_offsets (problem p's nq + 1 offsets at q0 + p); scal = [total, longest row, fits].  Sums in 64 bits,
// stored saturated: where they do not fit an int the verdict is 0 and nobody follows them.
constexpr int SCAN_T = 1024;
__global__ __launch_bounds__(SCAN_T) void radius_scan_kernel(MatchBatch b, int nprob, int nsplit, int *__restrict__ counts,
                                                             int *__restrict__ row_start, int *__restrict__ row_offsets,
                                                             int capacity, int *__restrict__ scal)
{
    __shared__ unsigned long long s_wave[SCAN_T / 64];
    __shared__ int longest;
    const int tid = threadIdx.x;
    if (tid == 0)
        longest = 0;
    unsigned long long carry = 0;
    for (int p = 0; p < nprob; p++) {
        const MatchProb pr = b.p[p];
        for (int base = 0; base < pr.nq; base += SCAN_T) {
            const int i = base + tid;
            int n = 0;
            if (i < pr.nq) {
                int *c = counts + (size_t)(pr.q0 + i) * nsplit;
                for (int s = 0; s < nsplit; s++) {
                    const int v = c[s];
                    c[s] = n;
                    n += v;  // at most the train rows of the problem
                }
            }
            __syncthreads();  // s_wave of the previous round has been read
            unsigned long long total;
            const unsigned long long before = svo::block_excl_scan<SCAN_T>((unsigned long long)n, s_wave, &total);
            if (i < pr.nq) {
                const int start = match_plan::saturate(carry + before);
                row_start[pr.q0 + i] = start;
                row_offsets[pr.q0 + i + p] = start;
                atomicMax(&longest, n);
            }
            carry += total;
        }
        if (tid == 0)
            row_offsets[pr.q0 + pr.nq + p] = match_plan::saturate(carry);
    }
    __syncthreads();
    if (tid == 0) {
        row_start[b.p[nprob - 1].q0 + b.p[nprob - 1].nq] = match_plan::saturate(carry);
        scal[0] = match_plan::saturate(carry);
        scal[1] = longest;
        scal[2] = match_plan::csr_fits(carry, longest, capacity);
    }
}

// grid: (queries, problems), one workgroup per query: its entries into LDS, padded with EMPTY to a power of two, a bitonic sort
// (entries are unique: any correct sort gives the one order), then idx / dist
__global__ __launch_bounds__(256) void radius_sort_kernel(MatchBatch b, const int *__restrict__ row_start,
                                                          const unsigned long long *__restrict__ entries,
                                                          const int *__restrict__ scal, int norm, int *__restrict__ idx,
                                                          float *__restrict__ dist)
{
    extern __shared__ __align__(16) unsigned long long se[];
    const MatchProb pr = b.p[blockIdx.y];
    if ((int)blockIdx.x >= pr.nq || scal[2] == 0)
        return;
    const int start = row_start[pr.q0 + blockIdx.x], n = row_start[pr.q0 + blockIdx.x + 1] - start;
    if (n <= 0)
        return;
    const int P = match_plan::sort_width(n);  // <= the launch's LDS: n <= min(train rows, SVO_RADIUS_MAX_PER_QUERY)
    for (int e = threadIdx.x; e < P; e += 256)
        se[e] = e < n ? entries[(size_t)start + e] : EMPTY;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int e = threadIdx.x; e < P; e += 256) {
                const int l = e ^ j;
                if (l > e) {
                    const unsigned long long a = se[e], c = se[l];
                    if ((a > c) == ((e & k) == 0)) {
                        se[e] = c;
                        se[l] = a;
                    }
                }
            }
            __syncthreads();
        }
    for (int e = threadIdx.x; e < n; e += 256) {
        idx[(size_t)start + e] = (int)(unsigned)se[e];
        dist[(size_t)start + e] = dist_of(norm, (unsigned)(se[e] >> 32));
    }
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

// ---- the host side shared by svo_match_cross, svo_radius_match and svo_knn_match_gated -----------------------------------
// the arguments the three have in common with svo_knn_match, decided before the context is touched
struct Common {
    int W, qlo, qhi, tlo, thi;
};
int check_common(const char *fn, svo_ctx *ctx, int norm, const void *query, const void *train, int dim, const int *q_offsets,
                 const int *t_offsets, int nprob, int mem, Common *c)
{
    SVO_CHECK_ARG(ctx && (mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE));
    SVO_CHECK_ARG(nprob >= 1 && nprob <= SVO_LK_MAX_JOBS);
    c->W = match_plan::words(norm, dim);
    SVO_CHECK_ARG(c->W > 0 /* an unknown norm, or a dim it does not take */);
    bool too_big = false;
    const char *why = match_plan::check_offsets(q_offsets, nprob, &c->qlo, &c->qhi, &too_big);
    if (!why)
        why = match_plan::check_offsets(t_offsets, nprob, &c->tlo, &c->thi, &too_big);
    if (why) {
        svo_set_error("%s: %s", fn, why);
        return SVO_ERR_ARG;
    }
    SVO_CHECK_ARG(c->qhi == c->qlo || query);
    SVO_CHECK_ARG(c->thi == c->tlo || train);
    SVO_CHECK_ARG((reinterpret_cast<uintptr_t>(query) & 3) == 0 && (reinterpret_cast<uintptr_t>(train) & 3) == 0);
    if (too_big) {
        svo_set_error("%s: at most %d queries and %d train rows per problem", fn, MAX_ROWS, MAX_ROWS);
        return SVO_ERR_CAPACITY;
    }
    return SVO_OK;
}

MatchBatch batch_of(const match_plan::Search &s)
{
    MatchBatch b;
    for (int p = 0; p < SVO_LK_MAX_JOBS; p++)
        b.p[p] = MatchProb{s.q0[p], s.nq[p], s.t0[p], s.nt[p]};
    return b;
}

// the descriptor rows on the device: the caller's own, or staged copies of the row ranges in use (s_a, s_b)
int stage_rows(svo_ctx *ctx, const Common &c, const void *query, const void *train, int mem, const uint32_t **dq,
               const uint32_t **dt)
{
    *dq = static_cast<const uint32_t *>(query);
    *dt = static_cast<const uint32_t *>(train);
    if (mem == SVO_MEM_DEVICE)
        return SVO_OK;
    const size_t row_b = (size_t)c.W * 4;
    int rc;
    if ((rc = ctx->s_a.ensure((size_t)(c.qhi > 0 ? c.qhi : 1) * row_b)) || (rc = ctx->s_b.ensure((size_t)(c.thi > 0 ? c.thi : 1) * row_b)))
        return rc;
    if (c.qhi > c.qlo)
        SVO_HIP(hipMemcpyAsync(ctx->s_a.as<char>() + (size_t)c.qlo * row_b, static_cast<const char *>(query) + (size_t)c.qlo * row_b,
                               (size_t)(c.qhi - c.qlo) * row_b, hipMemcpyHostToDevice, ctx->stream));
    if (c.thi > c.tlo)
        SVO_HIP(hipMemcpyAsync(ctx->s_b.as<char>() + (size_t)c.tlo * row_b, static_cast<const char *>(train) + (size_t)c.tlo * row_b,
                               (size_t)(c.thi - c.tlo) * row_b, hipMemcpyHostToDevice, ctx->stream));
    *dq = ctx->s_a.as<uint32_t>();
    *dt = ctx->s_b.as<uint32_t>();
    return SVO_OK;
}

// one launch of the tile loop over the problems of `s` (which has query rows); Q / T in the roles of `s`
template <int MODE>
void launch_search(svo_ctx *ctx, int norm, const match_plan::Search &s, int nprob, const uint32_t *Q, const uint32_t *T, int W,
                   unsigned long long *part, const SearchExtra &x)
{
    const int vec = (W % 4 == 0 && (reinterpret_cast<uintptr_t>(Q) & 15) == 0) ? 1 : 0;
    const int WP = (W + 3) & ~3;
    const size_t lds = (size_t)(MT * WP + MT + 2 * MT) * sizeof(uint32_t);
    const MatchBatch b = batch_of(s);
    const dim3 grid(s.qblocks_max, s.nsplit, nprob), block(MQ);
    if (norm == SVO_MATCH_L2_F32)
        hipLaunchKernelGGL((knn_partial_kernel<SVO_MATCH_L2_F32, MODE>), grid, block, lds, ctx->stream, b, Q, T, W, vec, s.nsplit, part, x);
    else if (norm == SVO_MATCH_L2_U8)
        hipLaunchKernelGGL((knn_partial_kernel<SVO_MATCH_L2_U8, MODE>), grid, block, lds, ctx->stream, b, Q, T, W, vec, s.nsplit, part, x);
    else
        hipLaunchKernelGGL((knn_partial_kernel<SVO_MATCH_HAMMING, MODE>), grid, block, lds, ctx->stream, b, Q, T, W, vec, s.nsplit, part, x);
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
    const SearchExtra none{};
    if (norm == SVO_MATCH_L2_F32)
        hipLaunchKernelGGL((knn_partial_kernel<SVO_MATCH_L2_F32, SEARCH_KNN>), grid, block, lds, ctx->stream, b, dq, dt, W, vec, nsplit,
                           part, none);
    else if (norm == SVO_MATCH_L2_U8)
        hipLaunchKernelGGL((knn_partial_kernel<SVO_MATCH_L2_U8, SEARCH_KNN>), grid, block, lds, ctx->stream, b, dq, dt, W, vec, nsplit,
                           part, none);
    else
        hipLaunchKernelGGL((knn_partial_kernel<SVO_MATCH_HAMMING, SEARCH_KNN>), grid, block, lds, ctx->stream, b, dq, dt, W, vec, nsplit,
                           part, none);
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

extern "C" int svo_knn_match_gated(svo_ctx *ctx, int norm, const void *query, const void *train, int dim, const int *q_offsets,
                                   const int *t_offsets, int nprob, int k, const uint8_t *mask, const float *xy_query,
                                   const float *xy_train, const svo_match_gate *gate, int *idx, float *dist, int mem)
{
    SVO_CHECK_ARG(ctx && k >= 1 && k <= 4);
    // exactly one form: the byte matrices, or the key points with their gate
    SVO_CHECK_ARG(mask ? (!xy_query && !xy_train && !gate) : (xy_query && xy_train && gate));
    Common c;
    int rc;
    if ((rc = check_common("svo_knn_match_gated", ctx, norm, query, train, dim, q_offsets, t_offsets, nprob, mem, &c)))
        return rc;
    SVO_CHECK_ARG(c.qhi == c.qlo || (idx && dist));
    if (c.qhi == c.qlo)
        return SVO_OK;  // no query anywhere: nothing is written
    const match_plan::Search s = match_plan::plan(q_offsets, t_offsets, nprob, false);
    if ((rc = ctx->w_a.ensure((size_t)c.qhi * s.nsplit * 4 * sizeof(unsigned long long))))
        return rc;
    const uint32_t *dq, *dt;
    if ((rc = stage_rows(ctx, c, query, train, mem, &dq, &dt)))
        return rc;
    int *didx = idx;
    float *ddist = dist;
    SearchExtra x{};
    uint64_t moff[SVO_LK_MAX_JOBS + 1];
    match_plan::mask_offsets(q_offsets, t_offsets, nprob, moff);
    for (int p = 0; p < nprob; p++)
        x.mask_off[p] = moff[p];
    x.mask = mask;
    x.xy_query = reinterpret_cast<const float2 *>(xy_query);
    x.xy_train = reinterpret_cast<const float2 *>(xy_train);
    if (gate)
        x.dy_max = gate->dy_max, x.dx_min = gate->dx_min, x.dx_max = gate->dx_max;
    if (mem == SVO_MEM_HOST) {
        if ((rc = ctx->s_c.ensure((size_t)c.qhi * k * 4)) || (rc = ctx->s_d.ensure((size_t)c.qhi * k * 4)))
            return rc;
        didx = ctx->s_c.as<int>();
        ddist = ctx->s_d.as<float>();
        if (mask) {
            if ((rc = ctx->s_e.ensure((size_t)(moff[nprob] > 0 ? moff[nprob] : 1))))
                return rc;
            if (moff[nprob] > 0)
                SVO_HIP(hipMemcpyAsync(ctx->s_e.p, mask, (size_t)moff[nprob], hipMemcpyHostToDevice, ctx->stream));
            x.mask = ctx->s_e.as<uint8_t>();
        } else {
            if ((rc = ctx->s_e.ensure((size_t)c.qhi * 8)) || (rc = ctx->s_f.ensure((size_t)(c.thi > 0 ? c.thi : 1) * 8)))
                return rc;
            SVO_HIP(hipMemcpyAsync(ctx->s_e.as<float>() + (size_t)c.qlo * 2, xy_query + (size_t)c.qlo * 2, (size_t)(c.qhi - c.qlo) * 8,
                                   hipMemcpyHostToDevice, ctx->stream));
            if (c.thi > c.tlo)
                SVO_HIP(hipMemcpyAsync(ctx->s_f.as<float>() + (size_t)c.tlo * 2, xy_train + (size_t)c.tlo * 2,
                                       (size_t)(c.thi - c.tlo) * 8, hipMemcpyHostToDevice, ctx->stream));
            x.xy_query = ctx->s_e.as<float2>();
            x.xy_train = ctx->s_f.as<float2>();
        }
    }
    unsigned long long *part = ctx->w_a.as<unsigned long long>();
    if (mask)
        launch_search<SEARCH_MASK>(ctx, norm, s, nprob, dq, dt, c.W, part, x);
    else
        launch_search<SEARCH_GATE>(ctx, norm, s, nprob, dq, dt, c.W, part, x);
    hipLaunchKernelGGL(knn_merge_kernel, dim3((s.nq_max + 255) / 256, nprob), dim3(256), 0, ctx->stream, batch_of(s), part, s.nsplit, k,
                       norm, didx, ddist);
    SVO_HIP(hipGetLastError());
    if (mem == SVO_MEM_DEVICE)
        return SVO_OK;
    const size_t o = (size_t)c.qlo * k, n = (size_t)(c.qhi - c.qlo) * k * 4;
    SVO_HIP(hipMemcpyAsync(idx + o, didx + o, n, hipMemcpyDeviceToHost, ctx->stream));
    SVO_HIP(hipMemcpyAsync(dist + o, ddist + o, n, hipMemcpyDeviceToHost, ctx->stream));
    SVO_HIP(hipStreamSynchronize(ctx->stream));
    return SVO_OK;
}

extern "C" int svo_match_cross(svo_ctx *ctx, int norm, const void *query, const void *train, int dim, const int *q_offsets,
                               const int *t_offsets, int nprob, int mode, int *idx, float *dist, int mem)
{
    SVO_CHECK_ARG(ctx && (mode == SVO_CROSS_MUTUAL || mode == SVO_CROSS_CV));
    Common c;
    int rc;
    if ((rc = check_common("svo_match_cross", ctx, norm, query, train, dim, q_offsets, t_offsets, nprob, mem, &c)))
        return rc;
    SVO_CHECK_ARG(c.qhi == c.qlo || (idx && dist));
    if (c.qhi == c.qlo)
        return SVO_OK;  // no query anywhere: nothing is written
    const match_plan::Search fwd = match_plan::plan(q_offsets, t_offsets, nprob, false);
    const match_plan::Search rev = match_plan::plan(q_offsets, t_offsets, nprob, true);
    const uint32_t *dq, *dt;
    if ((rc = stage_rows(ctx, c, query, train, mem, &dq, &dt)))
        return rc;
    int *didx = idx;
    float *ddist = dist;
    if (mem == SVO_MEM_HOST) {
        if ((rc = ctx->s_c.ensure((size_t)c.qhi * 4)) || (rc = ctx->s_d.ensure((size_t)c.qhi * 4)))
            return rc;
        didx = ctx->s_c.as<int>();
        ddist = ctx->s_d.as<float>();
    }
    const SearchExtra none{};
    if (c.thi == c.tlo) {
        hipLaunchKernelGGL(cross_none_kernel, dim3((c.qhi - c.qlo + 255) / 256), dim3(256), 0, ctx->stream, c.qlo, c.qhi, didx, ddist);
    } else {
        // the reverse search: every train row's best query
        if ((rc = ctx->w_d.ensure((size_t)c.thi * rev.nsplit * 4 * sizeof(unsigned long long))))
            return rc;
        unsigned long long *part_r = ctx->w_d.as<unsigned long long>();
        launch_search<SEARCH_KNN>(ctx, norm, rev, nprob, dt, dq, c.W, part_r, none);
        const dim3 qgrid((fwd.nq_max + 255) / 256, nprob), tgrid((rev.nq_max + 255) / 256, nprob);
        if (mode == SVO_CROSS_CV) {
            if ((rc = ctx->w_b.ensure((size_t)c.qhi * sizeof(unsigned long long))))
                return rc;
            unsigned long long *slot = ctx->w_b.as<unsigned long long>();
            SVO_HIP(hipMemsetAsync(slot + c.qlo, 0xff, (size_t)(c.qhi - c.qlo) * sizeof(unsigned long long), ctx->stream));  // EMPTY
            hipLaunchKernelGGL(cross_cv_kernel, tgrid, dim3(256), 0, ctx->stream, batch_of(rev), part_r, rev.nsplit, slot);
            hipLaunchKernelGGL(cross_finish_kernel, qgrid, dim3(256), 0, ctx->stream, batch_of(fwd), slot, norm, didx, ddist);
        } else {
            if ((rc = ctx->w_a.ensure((size_t)c.qhi * fwd.nsplit * 4 * sizeof(unsigned long long))))
                return rc;
            unsigned long long *part_f = ctx->w_a.as<unsigned long long>();
            launch_search<SEARCH_KNN>(ctx, norm, fwd, nprob, dq, dt, c.W, part_f, none);
            hipLaunchKernelGGL(cross_mutual_kernel, qgrid, dim3(256), 0, ctx->stream, batch_of(fwd), part_f, fwd.nsplit, part_r,
                               rev.nsplit, norm, didx, ddist);
        }
    }
    SVO_HIP(hipGetLastError());
    if (mem == SVO_MEM_DEVICE)
        return SVO_OK;
    const size_t n = (size_t)(c.qhi - c.qlo) * 4;
    SVO_HIP(hipMemcpyAsync(idx + c.qlo, didx + c.qlo, n, hipMemcpyDeviceToHost, ctx->stream));
    SVO_HIP(hipMemcpyAsync(dist + c.qlo, ddist + c.qlo, n, hipMemcpyDeviceToHost, ctx->stream));
    SVO_HIP(hipStreamSynchronize(ctx->stream));
    return SVO_OK;
}

extern "C" int svo_radius_match(svo_ctx *ctx, int norm, const void *query, const void *train, int dim, const int *q_offsets,
                                const int *t_offsets, int nprob, float max_distance, int *row_offsets, int *idx, float *dist,
                                int capacity, int *total, int mem)
{
    SVO_CHECK_ARG(ctx && !std::isnan(max_distance) && capacity >= 0 && row_offsets && total);
    SVO_CHECK_ARG(capacity == 0 || (idx && dist));
    Common c;
    int rc;
    if ((rc = check_common("svo_radius_match", ctx, norm, query, train, dim, q_offsets, t_offsets, nprob, mem, &c)))
        return rc;
    const match_plan::Search s = match_plan::plan(q_offsets, t_offsets, nprob, false);
    const int n_off = c.qhi - c.qlo + nprob;  // offsets in use: row_offsets[qlo .. qhi + nprob)
    if ((rc = ctx->w_a.ensure((size_t)(c.qhi > 0 ? c.qhi : 1) * s.nsplit * sizeof(int))) || (rc = ctx->w_b.ensure((size_t)(c.qhi + 1) * sizeof(int))) ||
        (rc = ctx->w_c.ensure(64)) || (rc = ctx->w_d.ensure((size_t)(capacity > 0 ? capacity : 1) * sizeof(unsigned long long))))
        return rc;
    const uint32_t *dq, *dt;
    if ((rc = stage_rows(ctx, c, query, train, mem, &dq, &dt)))
        return rc;
    int *doff = row_offsets, *didx = idx;
    float *ddist = dist;
    if (mem == SVO_MEM_HOST) {
        if ((rc = ctx->s_c.ensure((size_t)(c.qhi + nprob) * 4)) || (rc = ctx->s_d.ensure((size_t)(capacity > 0 ? capacity : 1) * 4)) ||
            (rc = ctx->s_e.ensure((size_t)(capacity > 0 ? capacity : 1) * 4)))
            return rc;
        doff = ctx->s_c.as<int>();
        didx = ctx->s_d.as<int>();
        ddist = ctx->s_e.as<float>();
    }
    SearchExtra x{};
    x.key_max = match_plan::radius_key_max(norm, max_distance);
    x.counts = ctx->w_a.as<int>();
    x.row_start = ctx->w_b.as<int>();
    x.scal = ctx->w_c.as<int>();
    x.entries = ctx->w_d.as<unsigned long long>();
    const MatchBatch b = batch_of(s);
    if (c.qhi > c.qlo)
        launch_search<SEARCH_COUNT>(ctx, norm, s, nprob, dq, dt, c.W, nullptr, x);
    hipLaunchKernelGGL(radius_scan_kernel, dim3(1), dim3(SCAN_T), 0, ctx->stream, b, nprob, s.nsplit, x.counts, ctx->w_b.as<int>(), doff,
                       capacity, ctx->w_c.as<int>());
    if (c.qhi > c.qlo) {
        launch_search<SEARCH_WRITE>(ctx, norm, s, nprob, dq, dt, c.W, nullptr, x);
        hipLaunchKernelGGL(radius_sort_kernel, dim3(s.nq_max, nprob), dim3(256), match_plan::sort_lds(s.nt_max), ctx->stream, b,
                           x.row_start, x.entries, x.scal, norm, didx, ddist);
    }
    SVO_HIP(hipGetLastError());
    int *back = reinterpret_cast<int *>(ctx->pinned);
    SVO_HIP(hipMemcpyAsync(back, ctx->w_c.p, 3 * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    if (mem == SVO_MEM_HOST)
        SVO_HIP(hipMemcpyAsync(row_offsets + c.qlo, doff + c.qlo, (size_t)n_off * 4, hipMemcpyDeviceToHost, ctx->stream));
    SVO_HIP(hipStreamSynchronize(ctx->stream));  // the one wait
    const int found = back[0], longest = back[1], fits = back[2];
    *total = found;
    if (!fits) {
        svo_set_error("svo_radius_match: %d matches (the longest row %d) for a capacity of %d and at most %d per query", found, longest,
                      capacity, SVO_RADIUS_MAX_PER_QUERY);
        return SVO_ERR_CAPACITY;
    }
    if (mem == SVO_MEM_HOST && found > 0) {
        SVO_HIP(hipMemcpyAsync(idx, didx, (size_t)found * 4, hipMemcpyDeviceToHost, ctx->stream));
        SVO_HIP(hipMemcpyAsync(dist, ddist, (size_t)found * 4, hipMemcpyDeviceToHost, ctx->stream));
        SVO_HIP(hipStreamSynchronize(ctx->stream));
    }
    return SVO_OK;
}
