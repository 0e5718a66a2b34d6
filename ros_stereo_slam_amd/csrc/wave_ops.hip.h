// wave_ops.hip.h -- the lowest layer every kernel file shares: reductions over the 64 lanes of a wavefront, the
// hand-off of LDS data inside one wave and the fixed-order sums of a 256-thread block.  Results are held bit for bit
// against the oracle, so the ORDER of every reduction here is part of its contract: do not change one in place.
#pragma once
#include <hip/hip_runtime.h>

namespace svo {

// LDS produced by some lanes of a wave and consumed by others of the SAME wave: LDS
// instructions of one wave execute in order; this only stops the compiler from moving
// accesses across the hand-off.
__device__ __forceinline__ void wave_lds_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- sums -----------------------------------------------------------------------------------------------------------
// Two forms; a call site keeps the one it has (they are different instructions).
//   wave_sum      shuffle butterfly, any of int / long long / double, every lane gets the total.  The order -- offsets
//                 32, 16, .. 1 -- is part of the contract: it is the tree the double-precision callers are compared on.
//   wave_sum_dpp  int only, DPP inside the 16-lane rows and the four row totals added on the scalar unit: exact while
//                 the total of the per-lane values has no carry out of 32 bits; the result is wave-uniform (an SGPR).
template <class T> __device__ __forceinline__ T wave_sum(T v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
        v += __shfl_xor(v, off, 64);
    return v;
}

// every lane gets the total of its 16-lane row
__device__ __forceinline__ int row16_sum(int v)
{
    v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, false);   // quad_perm [1,0,3,2]
    v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xf, 0xf, false);   // quad_perm [2,3,0,1]
    v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xf, 0xf, false);  // row_half_mirror
    v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xf, 0xf, false);  // row_mirror
    return v;
}

__device__ __forceinline__ int wave_sum_dpp(int v)
{
    v = row16_sum(v);
    return __builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16) +
           __builtin_amdgcn_readlane(v, 32) + __builtin_amdgcn_readlane(v, 48);
}

// ---- minimum / maximum: offsets 32, 16, .. 1, every lane gets the result ---------------------------------------------
__device__ __forceinline__ int wave_min(int v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
        v = min(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ int wave_max(int v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
        v = max(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ float wave_min(float v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
        v = fminf(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ float wave_max(float v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
        v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ double wave_min(double v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
        v = fmin(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ double wave_max(double v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
        v = fmax(v, __shfl_xor(v, off, 64));
    return v;
}

// ---- blocks of 256 threads --------------------------------------------------------------------------------------------
// K per-thread partials -> K totals in every thread, fixed order: balanced tree inside each
// wavefront (xor butterfly, commutative additions: every lane holds the same bits), then the four
// wave totals ((w0 + w1) + w2) + w3 through LDS.
template <int K> __device__ __forceinline__ void block_sum(double (&v)[K], double *s_red /* [4][K] */)
{
#pragma unroll
    for (int k = 0; k < K; k++) {
        double x = v[k];
#pragma unroll
        for (int m = 1; m < 64; m <<= 1)
            x = x + __shfl_xor(x, m, 64);
        v[k] = x;
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();  // the previous reduction's readers are done with s_red
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < K; k++)
            s_red[wave * K + k] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; k++)
        v[k] = ((s_red[k] + s_red[K + k]) + s_red[2 * K + k]) + s_red[3 * K + k];
}

__device__ __forceinline__ double block_max(double x, double *s_red)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1)
        x = fmax(x, __shfl_xor(x, m, 64));
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();
    if (lane == 0)
        s_red[wave] = x;
    __syncthreads();
    return fmax(fmax(s_red[0], s_red[1]), fmax(s_red[2], s_red[3]));
}

}  // namespace svo
