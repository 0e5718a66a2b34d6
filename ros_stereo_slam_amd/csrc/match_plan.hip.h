// match_plan.hip.h -- the host arithmetic of match.hip's cross-check, radius and gated searches with nothing of the HIP runtime in
// it: the words of a row, the offset checks and the 32768-row refusal, the split of a train range over workgroups, the largest
// selection key a radius admits, where a problem's byte mask starts, the CSR verdict and the width of one query's sort.  match.hip
// includes it; so does tests/cpp/match_plan_check.cpp, a stand-alone program that runs it under the address and
// undefined-behaviour sanitizers.
#pragma once

#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../include/svo.h"

#if defined(__HIPCC__)
#define MATCH_PLAN_HD __host__ __device__
#else
#define MATCH_PLAN_HD
#endif

namespace match_plan {

constexpr int MT = 32;           // train rows per LDS tile = accumulators per lane
constexpr int MQ = 256;          // queries per workgroup, one per lane
constexpr int MAX_ROWS = 32768;  // queries / train rows per problem
constexpr int MAX_SPLIT = 64;    // workgroups one query's train range is split over at most
constexpr int TARGET_GROUPS = 1024;
constexpr int MAX_PROB = 16;     // SVO_LK_MAX_JOBS
// matches one query of svo_radius_match may have: its sort holds them in LDS as 64-bit (key, index) entries, 8192 x 8 = 64 KB,
// so that two workgroups sort side by side in the 160 KB of a CU
constexpr int RADIUS_MAX_PER_QUERY = SVO_RADIUS_MAX_PER_QUERY;
static_assert((RADIUS_MAX_PER_QUERY & (RADIUS_MAX_PER_QUERY - 1)) == 0 && RADIUS_MAX_PER_QUERY * 8 * 2 <= 160 * 1024, "LDS");

// 32-bit words of a row; 0: the norm or the dim is refused
inline int words(int norm, int dim)
{
    if (norm == SVO_MATCH_L2_F32)
        return dim >= 1 && dim <= 256 ? dim : 0;
    if (norm == SVO_MATCH_L2_U8)
        return dim >= 4 && dim <= 256 && dim % 4 == 0 ? dim / 4 : 0;
    if (norm == SVO_MATCH_HAMMING)
        return dim >= 1 && dim <= 16 ? dim : 0;
    return 0;
}

// nprob + 1 ascending offsets from a non-negative start.  0 = fine, else the reason; *too_big is SET (never cleared) when a
// problem has more than MAX_ROWS rows
inline const char *check_offsets(const int *off, int nprob, int *lo, int *hi, bool *too_big)
{
    if (!off)
        return "the offset arrays must not be null";
    if (off[0] < 0)
        return "offsets must not be negative";
    for (int p = 0; p < nprob; p++) {
        if (off[p + 1] < off[p])
            return "offsets must not decrease";
        if (off[p + 1] - off[p] > MAX_ROWS)
            *too_big = true;
    }
    *lo = off[0];
    *hi = off[nprob];
    return nullptr;
}

// one search: its problems (the roles swapped for a reverse search) and its launch geometry.  The split is svo_knn_match's:
// enough workgroups to fill the device, never more than MAX_SPLIT or than the tiles of the longest train range, at least one
struct Search {
    int q0[MAX_PROB], nq[MAX_PROB], t0[MAX_PROB], nt[MAX_PROB];
    int qblocks, qblocks_max, tiles_max, nq_max, nt_max, nsplit;
};
inline Search plan(const int *q_offsets, const int *t_offsets, int nprob, bool swap)
{
    Search s;
    memset(&s, 0, sizeof s);
    const int *qo = swap ? t_offsets : q_offsets, *to = swap ? q_offsets : t_offsets;
    for (int p = 0; p < MAX_PROB; p++) {
        const int k = p < nprob ? p : 0;  // the unused slots repeat problem 0: no kernel reads them
        s.q0[p] = qo[k], s.nq[p] = qo[k + 1] - qo[k], s.t0[p] = to[k], s.nt[p] = to[k + 1] - to[k];
        if (p >= nprob)
            continue;
        const int qb = (s.nq[p] + MQ - 1) / MQ, tl = (s.nt[p] + MT - 1) / MT;
        s.qblocks += qb;
        s.qblocks_max = qb > s.qblocks_max ? qb : s.qblocks_max;
        s.tiles_max = tl > s.tiles_max ? tl : s.tiles_max;
        s.nq_max = s.nq[p] > s.nq_max ? s.nq[p] : s.nq_max;
        s.nt_max = s.nt[p] > s.nt_max ? s.nt[p] : s.nt_max;
    }
    int n = s.qblocks > 0 ? (TARGET_GROUPS + s.qblocks - 1) / s.qblocks : 1;
    n = n > MAX_SPLIT ? MAX_SPLIT : n;
    n = n > s.tiles_max ? s.tiles_max : n;
    s.nsplit = n < 1 ? 1 : n;
    return s;
}

// dist of a key, as the kernels form it: the double root of a float (or of an integer below 2^24) rounded to float is the
// correctly rounded float root
inline float dist_of_key(int norm, uint32_t key)
{
    if (norm == SVO_MATCH_L2_F32) {
        float s;
        memcpy(&s, &key, 4);
        return (float)sqrt((double)s);
    }
    return norm == SVO_MATCH_L2_U8 ? (float)sqrt((double)key) : (float)key;
}

// svo_radius_match compares the RETURNED float: dist <= max_distance.  dist is a monotone function of the key, so the keys that
// pass are the keys up to a largest one, found here once per call; the kernels compare keys.  -1: no key passes (a negative or
// NaN radius).  The float norm's key is the bit pattern of a non-negative float (ordered like the floats; the NaN key 0x7fc00000
// lies above +inf's 0x7f800000 and never passes); the integer keys go up to 256 * 255^2 < 2^24.
inline int64_t radius_key_max(int norm, float r)
{
    if (!(r >= 0.f))
        return -1;
    if (norm == SVO_MATCH_HAMMING)
        return r >= 512.f ? 512 : (int64_t)floorf(r);  // 16 words hold 512 bits
    if (norm == SVO_MATCH_L2_U8) {
        const int64_t top = (1 << 24) - 1;
        const double sq = (double)r * (double)r;
        int64_t k = sq >= (double)top ? top : (int64_t)sq;
        while (k > 0 && dist_of_key(norm, (uint32_t)k) > r)
            k--;
        while (k < top && dist_of_key(norm, (uint32_t)(k + 1)) <= r)
            k++;
        return k;
    }
    float s = (float)((double)r * (double)r);  // +inf when it overflows
    uint32_t k;
    memcpy(&k, &s, 4);
    while (k > 0 && dist_of_key(norm, k) > r)
        k--;  // the next float below: non-negative floats order as their bit patterns
    while (k < 0x7f800000u && dist_of_key(norm, k + 1) <= r)
        k++;
    return (int64_t)k;
}

// the byte masks of svo_knn_match_gated lie back to back, problem p's nq_p x nt_p matrix at off[p]; off[nprob]: bytes in all
inline void mask_offsets(const int *q_offsets, const int *t_offsets, int nprob, uint64_t *off)
{
    off[0] = 0;
    for (int p = 0; p < nprob; p++)
        off[p + 1] = off[p] + (uint64_t)(q_offsets[p + 1] - q_offsets[p]) * (uint64_t)(t_offsets[p + 1] - t_offsets[p]);
}

MATCH_PLAN_HD inline int saturate(uint64_t v) { return v > (uint64_t)INT_MAX ? INT_MAX : (int)v; }

// what the scan of svo_radius_match decides from the total and the longest row: 1 = the matches are written
MATCH_PLAN_HD inline int csr_fits(uint64_t total, int max_row, int capacity)
{
    return capacity >= 0 && total <= (uint64_t)capacity && max_row <= RADIUS_MAX_PER_QUERY ? 1 : 0;
}

// entries one query's sort is padded to: the power of two at or above n (n: 1..RADIUS_MAX_PER_QUERY)
MATCH_PLAN_HD inline int sort_width(int n)
{
    int p = 1;
    while (p < n)
        p <<= 1;
    return p;
}

// LDS bytes of the sort launch: no row is longer than the longest train range or than the bound
inline size_t sort_lds(int nt_max)
{
    const int n = nt_max < 1 ? 1 : nt_max > RADIUS_MAX_PER_QUERY ? RADIUS_MAX_PER_QUERY : nt_max;
    return (size_t)sort_width(n) * 8;
}

}  // namespace match_plan
