// cloud_index.hip.h -- the spatial index of a large cloud, shared by sor_grid.hip (svo_sor_filter_large) and cloud.hip
// (svo_cloud, the ICP): 63-bit Morton keys on a 2^21 grid per axis, the stable LSD radix sort of (key, index) pairs, the
// gather into Morton order, the 64-way box hierarchy over the sorted array and the lower bound of the squared distance
// of a point to a box.  Every kernel here has internal linkage: each of the two translation units carries its own copy.
#pragma once
#include "svo_internal.h"
#include "scan_ops.hip.h"
#include "wave_ops.hip.h"

namespace {

// ---- stable LSD radix sort of (uint64 key, int value) pairs ------------------------------------------------------
// A tile of RS_TILE elements per workgroup.  Per pass: a digit histogram per tile, one exclusive scan over
// (digit, tile), then a scatter that ranks every element among the equal digits of its tile in element order (lane
// order inside a wave by ballot matching, wave order inside a round, round order inside the tile).
constexpr int RS_THREADS = 256, RS_ROUNDS = 16, RS_TILE = RS_THREADS * RS_ROUNDS;

// lanes of this wave that hold the same 8-bit digit (valid lanes only)
__device__ __forceinline__ unsigned long long match_digit(bool valid, unsigned d)
{
    unsigned long long peers = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; b++) {
        const bool on = (d >> b) & 1u;
        const unsigned long long bb = __ballot(on);
        peers &= on ? bb : ~bb;
    }
    return peers;
}

__global__ __launch_bounds__(RS_THREADS) void radix_hist_kernel(const uint64_t *__restrict__ keys, int n, int shift,
                                                                int nblk, unsigned *__restrict__ hist)
{
    __shared__ unsigned h[256];
    const int tid = threadIdx.x;
    h[tid] = 0;
    __syncthreads();
    const int base = blockIdx.x * RS_TILE;
    for (int r = 0; r < RS_ROUNDS; r++) {
        const int i = base + r * RS_THREADS + tid;
        const bool valid = i < n;
        const unsigned d = valid ? (unsigned)(keys[i] >> shift) & 255u : 0u;
        const unsigned long long peers = match_digit(valid, d);
        if (valid && svo::lanes_below(peers) == 0)  // the lowest lane of its digit adds for all of them
            atomicAdd(&h[d], (unsigned)__popcll(peers));
    }
    __syncthreads();
    hist[tid * nblk + blockIdx.x] = h[tid];
}

// exclusive scan of total (= 256 x nblk, digit-major) counts in place, one workgroup: `per` counts a thread, the block scan of
// scan_ops.hip.h over the threads' sums, the counts again
__global__ __launch_bounds__(1024) void radix_scan_kernel(unsigned *__restrict__ h, int total)
{
    __shared__ unsigned s_wave[16];
    const int tid = threadIdx.x;
    const int per = (total + 1023) / 1024;
    const int s = tid * per, e = min(s + per, total);
    unsigned sum = 0;
    for (int j = s; j < e; j++)
        sum += h[j];
    unsigned run = svo::block_excl_scan<1024>(sum, s_wave, (unsigned *)nullptr);
    for (int j = s; j < e; j++) {
        const unsigned t = h[j];
        h[j] = run;
        run += t;
    }
}

__global__ __launch_bounds__(RS_THREADS) void radix_scatter_kernel(const uint64_t *__restrict__ kin,
                                                                   const int *__restrict__ vin,
                                                                   uint64_t *__restrict__ kout, int *__restrict__ vout,
                                                                   int n, int shift, int nblk,
                                                                   const unsigned *__restrict__ hist)
{
    __shared__ unsigned run[256];
    __shared__ unsigned wcnt[RS_THREADS / 64][256];
    const int tid = threadIdx.x, w = tid >> 6;
    run[tid] = hist[tid * nblk + blockIdx.x];
#pragma unroll
    for (int q = 0; q < RS_THREADS / 64; q++)
        wcnt[q][tid] = 0;
    __syncthreads();
    const int base = blockIdx.x * RS_TILE;
    for (int r = 0; r < RS_ROUNDS && base + r * RS_THREADS < n; r++) {  // the bound is uniform over the workgroup
        const int i = base + r * RS_THREADS + tid;
        const bool valid = i < n;
        const uint64_t key = valid ? kin[i] : 0ull;
        const unsigned d = (unsigned)(key >> shift) & 255u;
        const unsigned long long peers = match_digit(valid, d);
        const int rank = svo::lanes_below(peers);
        if (valid && rank == 0)
            wcnt[w][d] = (unsigned)__popcll(peers);
        __syncthreads();
        if (valid) {
            unsigned pos = run[d] + (unsigned)rank;
            for (int q = 0; q < w; q++)
                pos += wcnt[q][d];
            kout[pos] = key;
            vout[pos] = vin[i];
        }
        __syncthreads();
        unsigned add = 0;
#pragma unroll
        for (int q = 0; q < RS_THREADS / 64; q++) {
            add += wcnt[q][tid];
            wcnt[q][tid] = 0;
        }
        run[tid] += add;
        __syncthreads();
    }
}

// sorts k0/v0 in place (8 passes over the 64-bit keys, k1/v1 the ping-pong buffers); hist: 256 x ceil(n / RS_TILE)
int radix_sort_pairs(hipStream_t st, uint64_t *k0, int *v0, uint64_t *k1, int *v1, int n, unsigned *hist)
{
    if (n <= 0)
        return SVO_OK;
    const int nblk = (n + RS_TILE - 1) / RS_TILE;
    for (int pass = 0; pass < 8; pass++) {
        const int shift = 8 * pass;
        const uint64_t *ki = pass & 1 ? k1 : k0;
        const int *vi = pass & 1 ? v1 : v0;
        uint64_t *ko = pass & 1 ? k0 : k1;
        int *vo = pass & 1 ? v0 : v1;
        hipLaunchKernelGGL(radix_hist_kernel, dim3(nblk), dim3(RS_THREADS), 0, st, ki, n, shift, nblk, hist);
        hipLaunchKernelGGL(radix_scan_kernel, dim3(1), dim3(1024), 0, st, hist, 256 * nblk);
        hipLaunchKernelGGL(radix_scatter_kernel, dim3(nblk), dim3(RS_THREADS), 0, st, ki, vi, ko, vo, n, shift, nblk,
                           hist);
    }
    SVO_HIP(hipGetLastError());
    return SVO_OK;
}

// ---- the cloud: pre-filter, bounds, keys, Morton order, box hierarchy ---------------------------------------------
__global__ __launch_bounds__(256) void sorg_zmask_kernel(const float *__restrict__ xyz, int n, float z_limit,
                                                         uint8_t *__restrict__ mask)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
        const bool finite = isfinite(x) && isfinite(y) && isfinite(z);
        mask[i] = (!finite || (z_limit > 0.f && -1.f * z > z_limit)) ? 0 : 1;
    }
}

// bnd: lo x, y, z, cells per unit (doubles); one workgroup
__global__ __launch_bounds__(1024) void sorg_bounds_kernel(const float *__restrict__ xyz, const int *__restrict__ d_m,
                                                           double *__restrict__ bnd)
{
    __shared__ float s_lo[3][1024], s_hi[3][1024];
    const int m = *d_m, tid = threadIdx.x;
    float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()};
    float hi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    for (int i = tid; i < m; i += 1024)
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const float v = xyz[3 * i + a];
            lo[a] = fminf(lo[a], v);
            hi[a] = fmaxf(hi[a], v);
        }
#pragma unroll
    for (int a = 0; a < 3; a++) {
        s_lo[a][tid] = lo[a];
        s_hi[a][tid] = hi[a];
    }
    __syncthreads();
    for (int off = 512; off >= 1; off >>= 1) {
        if (tid < off)
#pragma unroll
            for (int a = 0; a < 3; a++) {
                s_lo[a][tid] = fminf(s_lo[a][tid], s_lo[a][tid + off]);
                s_hi[a][tid] = fmaxf(s_hi[a][tid], s_hi[a][tid + off]);
            }
        __syncthreads();
    }
    if (tid == 0) {
        double ext = 0;
        for (int a = 0; a < 3; a++) {
            const double e = m > 0 ? (double)s_hi[a][0] - (double)s_lo[a][0] : 0.0;
            ext = e > ext ? e : ext;
            bnd[a] = m > 0 ? (double)s_lo[a][0] : 0.0;
        }
        bnd[3] = ext > 0 ? 2097152.0 / ext : 0.0;
    }
}

__device__ __forceinline__ uint64_t spread3_21(uint64_t x)
{
    x &= 0x1fffffull;
    x = (x | x << 32) & 0x1f00000000ffffull;
    x = (x | x << 16) & 0x1f0000ff0000ffull;
    x = (x | x << 8) & 0x100f00f00f00f00full;
    x = (x | x << 4) & 0x10c30c30c30c30c3ull;
    x = (x | x << 2) & 0x1249249249249249ull;
    return x;
}

// keys of the m points; slots m..n-1 get the largest key (they sort last); values: the point's index
__global__ __launch_bounds__(256) void sorg_key_kernel(const float *__restrict__ xyz, const int *__restrict__ d_m,
                                                       const double *__restrict__ bnd, int n, uint64_t *__restrict__ keys,
                                                       int *__restrict__ vals)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    uint64_t key = ~0ull;
    if (i < *d_m) {
        const double inv = bnd[3];
        uint64_t c[3];
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const double q = floor(((double)xyz[3 * i + a] - bnd[a]) * inv);
            c[a] = q <= 0.0 ? 0ull : (q >= 2097151.0 ? 2097151ull : (uint64_t)q);
        }
        key = spread3_21(c[0]) | spread3_21(c[1]) << 1 | spread3_21(c[2]) << 2;
    }
    keys[i] = key;
    vals[i] = i;
}

__global__ __launch_bounds__(256) void sorg_gather_kernel(const float *__restrict__ xyz, const int *__restrict__ idx,
                                                          const int *__restrict__ d_m, int n, float *__restrict__ pts)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || i >= *d_m)
        return;
    const int j = idx[i];
    pts[3 * i] = xyz[3 * j];
    pts[3 * i + 1] = xyz[3 * j + 1];
    pts[3 * i + 2] = xyz[3 * j + 2];
}

// number of elements at a level of the hierarchy: 0 = points, 1..3 = boxes
__device__ __forceinline__ int level_count(int m, int level)
{
    for (int l = 0; l < level; l++)
        m = (m + 63) >> 6;
    return m;
}

// one wave per box of `level` (1..3): the bounds of its 64 children (points for level 1, boxes below), as
// lo x, y, z, hi x, y, z
__global__ __launch_bounds__(256) void sorg_box_kernel(const float *__restrict__ child, const int *__restrict__ d_m,
                                                       int level, int cap_boxes, float *__restrict__ box)
{
    const int b = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const int m = *d_m;
    const int nb = level_count(m, level), nc = level_count(m, level - 1);
    if (b >= nb || b >= cap_boxes)
        return;
    const int c = b * 64 + lane;
    float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()};
    float hi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    if (c < nc) {
        if (level == 1) {
#pragma unroll
            for (int a = 0; a < 3; a++)
                lo[a] = hi[a] = child[3 * c + a];
        } else {
#pragma unroll
            for (int a = 0; a < 3; a++) {
                lo[a] = child[6 * c + a];
                hi[a] = child[6 * c + 3 + a];
            }
        }
    }
#pragma unroll
    for (int a = 0; a < 3; a++) {
        lo[a] = svo::wave_min(lo[a]);
        hi[a] = svo::wave_max(hi[a]);
    }
    if (lane == 0)
#pragma unroll
        for (int a = 0; a < 3; a++) {
            box[6 * b + a] = lo[a];
            box[6 * b + 3 + a] = hi[a];
        }
}

// squared distance lower bound of any point of box b to (px, py, pz), in double
__device__ __forceinline__ double box_mind2(const float *__restrict__ box, int b, float px, float py, float pz)
{
    const float p[3] = {px, py, pz};
    double s = 0;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const double lo = box[6 * b + a], hi = box[6 * b + 3 + a], v = p[a];
        const double g = lo > v ? lo - v : (v > hi ? v - hi : 0.0);
        s += g * g;
    }
    return s;
}

__device__ __forceinline__ double shfl_double(double v, int src)
{
    return __shfl(v, src, 64);
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace
