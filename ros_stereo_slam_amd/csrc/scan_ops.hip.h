// scan_ops.hip.h -- the other half of wave_ops.hip.h: integer prefix sums over a wavefront and over a workgroup, the pieces
// under every ordered compaction (count per span, exclusive scan of the counts, every survivor written at its rank).
// Integer sums only: any correct scan gives the same bits, so nothing here is part of the bit-exact contract.
//
// Rules for callers:
//   * workgroups are one-dimensional and a multiple of 64 threads, so that threadIdx.x & 63 is the lane;
//   * EVERY thread of the workgroup calls waves_before / block_excl_scan / block_scan_counts (each holds a barrier);
//   * block_excl_scan and waves_before hold exactly ONE barrier, between the store of the wave totals and their reads.  A
//     caller that uses the same s_wave again puts a barrier of its own between the calls (the looped callers end every
//     round with one).
#pragma once
#include <hip/hip_runtime.h>

namespace svo {

// inclusive scan over the 64 lanes: shuffles up by 1, 2, ... 32
template <class T> __device__ __forceinline__ T wave_incl_scan(T v)
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T u = __shfl_up(v, o, 64);
        v += lane >= o ? u : T(0);
    }
    return v;
}

// the set bits of a ballot below the calling lane: the rank of a lane among the lanes that voted
__device__ __forceinline__ int lanes_below(unsigned long long ballot)
{
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)ballot, 0u));
}

// The sum of the totals of the waves before the caller's in its workgroup; *total (when not null) gets the sum over all
// waves.  wave_total must be right in lane 63 (a ballot's popcount is right in every lane).
template <int THREADS, class T> __device__ __forceinline__ T waves_before(T wave_total, T *s_wave /* [THREADS / 64] */, T *total)
{
    static_assert(THREADS % 64 == 0 && THREADS >= 64 && THREADS <= 1024, "whole waves, one workgroup");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 63)
        s_wave[wave] = wave_total;
    __syncthreads();
    T before = T(0), all = T(0);
#pragma unroll
    for (int k = 0; k < THREADS / 64; k++) {
        const T wt = s_wave[k];
        before += k < wave ? wt : T(0);
        all += wt;
    }
    if (total)
        *total = all;
    return before;
}

// the exclusive prefix of v over the workgroup's threads
template <int THREADS, class T> __device__ __forceinline__ T block_excl_scan(T v, T *s_wave /* [THREADS / 64] */, T *total)
{
    const T incl = wave_incl_scan(v);
    return waves_before<THREADS>(incl, s_wave, total) + incl - v;
}

// off[0 .. n) = the exclusive scan of cnt[0 .. n), in chunks of THREADS with a carry; every thread gets the total.
// off == cnt is allowed: a thread reads its element of a chunk before it writes it, and no other thread touches it.
template <int THREADS, class T> __device__ __forceinline__ T block_scan_counts(const T *cnt, T *off, int n, T *s_wave /* [THREADS / 64] */)
{
    T carry = T(0);
    for (int b = 0; b < n; b += THREADS) {   // n <= 2^31 - THREADS
        const int i = b + (int)threadIdx.x;
        const T v = i < n ? cnt[i] : T(0);
        T total;
        const T before = block_excl_scan<THREADS>(v, s_wave, &total);
        if (i < n)
            off[i] = carry + before;
        carry += total;
        __syncthreads();   // s_wave is free for the next chunk
    }
    return carry;
}

}  // namespace svo
