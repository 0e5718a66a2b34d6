// sor_common.hip.h -- device code shared by the two statistical outlier removal paths (sor.hip: brute force,
// sor_grid.hip: the Morton-ordered kNN): the cloud statistics.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

// mean / stddev of the distances in point order by one thread (PCL's own loop), then the keep mask.  The summing
// thread reads the distances from LDS: the other waves stage them SOR_STAGE at a time, one chunk ahead (two buffers),
// so the sequential chain of double adds is not also a chain of global-memory round trips (25 ms at 4.7e5 points
// with one global load per element).  The adds are the same, in the same order.
constexpr int SOR_STAGE = 4096;

__device__ __forceinline__ void sor_accumulate(float d, double &sum, double &sq_sum)
{
    sum += d;
    sq_sum += d * d;  // the product in float, as upstream
}

__global__ __launch_bounds__(1024) void sor_threshold_kernel(const float *__restrict__ dist,
                                                             const int *__restrict__ d_m, double stddev_mul, int cap,
                                                             uint8_t *__restrict__ mask)
{
    __shared__ float4 s_d[2][SOR_STAGE / 4];
    __shared__ double s_thr;
    const int m = *d_m, tid = threadIdx.x;
    const int nchunk = (m + SOR_STAGE - 1) / SOR_STAGE;
    float *s0 = reinterpret_cast<float *>(s_d[0]);
    for (int j = tid; j < SOR_STAGE && j < m; j += 1024)
        s0[j] = dist[j];
    __syncthreads();
    double sum = 0, sq_sum = 0;
    for (int c = 0; c < nchunk; c++) {  // wave 0 sums chunk c while waves 1.. stage chunk c + 1
        if (tid == 0) {
            const float4 *cur = s_d[c & 1];
            const int len = min(SOR_STAGE, m - c * SOR_STAGE);
            int j = 0;
            for (; j + 16 <= len; j += 16) {
                const float4 a = cur[j / 4], b = cur[j / 4 + 1], e = cur[j / 4 + 2], f = cur[j / 4 + 3];
                const float v[16] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, e.x, e.y, e.z, e.w, f.x, f.y, f.z, f.w};
#pragma unroll
                for (int q = 0; q < 16; q++)
                    sor_accumulate(v[q], sum, sq_sum);
            }
            const float *tail = reinterpret_cast<const float *>(cur);
            for (; j < len; j++)
                sor_accumulate(tail[j], sum, sq_sum);
        } else if (tid >= 64 && c + 1 < nchunk) {
            const int base = (c + 1) * SOR_STAGE;
            float *nxt = reinterpret_cast<float *>(s_d[(c + 1) & 1]);
            for (int j = tid - 64; j < SOR_STAGE && base + j < m; j += 1024 - 64)
                nxt[j] = dist[base + j];
        }
        __syncthreads();
    }
    if (tid == 0) {
        double thr = 1.7976931348623157e308;
        if (m > 1) {
            const double mean = sum / m;
            double variance = (sq_sum - sum * sum / m) / (m - 1);
            if (variance < 0)
                variance = 0;
            thr = mean + stddev_mul * sqrt(variance);
        }
        s_thr = thr;
    }
    __syncthreads();
    const double thr = s_thr;
    for (int i = threadIdx.x; i < cap; i += 1024)
        mask[i] = (i < m && (double)dist[i] <= thr) ? 1 : 0;
}

}  // namespace
