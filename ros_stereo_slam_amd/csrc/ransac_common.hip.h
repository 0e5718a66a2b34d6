// ransac_common.hip.h -- device helpers shared by the four RANSAC kernel files: fransac.hip (F matrix, 7-point samples),
// pnp.hip (PnP, 5), essential.hip (E matrix, 5) and homography.hip (H, 4): the counter-based generator, the draw of a sample, the iteration bound and
// the replay of the sequential loop.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>

#include "../../include/svo_math.h"  // sin / cos / acos / cbrt / log shared with the oracle, bit for bit
#include "wave_ops.hip.h"            // wave_sum_dpp (the inlier counts), wave_lds_fence

namespace svo {

// Counter-based generator: draw k of RANSAC iteration i is a pure function of
// (seed, i, k), so every iteration can be evaluated concurrently and the SEQUENTIAL
// algorithm (first-best-wins, adaptive iteration count) is reproduced afterwards.
__host__ __device__ __forceinline__ uint32_t rng_u32(uint64_t seed, uint32_t iter, uint32_t draw)
{
    uint64_t z = seed + 0x9E3779B97F4A7C15ull * ((((uint64_t)iter << 32) | draw) + 1ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (uint32_t)(z >> 32);
}

constexpr int kMaxAttempts = 8;
constexpr int kMaxDraws = 64;

// A sample of M distinct indices below n for RANSAC iteration `it` (orc_draw_subset_plain in the checker):
// slot by slot, a value that an earlier slot holds is drawn again; at most kMaxDraws draws per call.  false: a slot could not be
// filled.  The caller owns the draw counter: pnp_hypothesis and em_iter_kernel start it at 0, fr_solve_wave carries it on across
// its kMaxAttempts re-draws of a degenerate sample.
template <int M> __device__ __forceinline__ bool draw_distinct(uint64_t seed, int it, int n, uint32_t &draw, int (&idx)[M])
{
    int guard = 0;
    bool filled = true;
#pragma unroll
    for (int slot = 0; slot < M; slot++) {
        int v = 0;
        bool got = false;
        while (!got && guard < kMaxDraws) {
            v = (int)(rng_u32(seed, (uint32_t)it, draw++) % (uint32_t)n);
            guard++;
            bool dup = false;
#pragma unroll
            for (int j = 0; j < M; j++)
                if (j < slot && idx[j] == v)
                    dup = true;
            got = !dup;
        }
        if (!got)
            filled = false;
        idx[slot] = v;
    }
    return filled;
}

// cv RANSACUpdateNumIters
__device__ __forceinline__ int update_num_iters(double p, double ep, int model_points, int max_iters)
{
    p = p < 0 ? 0 : (p > 1 ? 1 : p);
    ep = ep < 0 ? 0 : (ep > 1 ? 1 : ep);
    double num = 1. - p;
    if (num < DBL_MIN)
        num = DBL_MIN;
    double denom = 1. - svo_powi(1. - ep, model_points);  // include/svo_math.h: the oracle runs the same operations
    if (denom < DBL_MIN)
        return 0;
    num = svo_log(num);
    denom = svo_log(denom);
    return denom >= 0 || -num >= max_iters * (-denom) ? max_iters : (int)rint(num / denom);
}

// running state of the sequential RANSAC loop, kept in HBM between the phase kernels
struct RansacState {
    int niters;      // current iteration bound (starts at max_iters)
    int next_iter;   // first iteration the select pass has not looked at yet
    int best_iter;   // -1 = none
    int best_model;
    int best_count;
    int done;        // 1: loop finished (next_iter >= niters or a subset draw failed)
    int iters_run;
    int pad;
};

// Replays the SEQUENTIAL RANSAC loop over iterations [st->next_iter, it_end) (called by one
// thread: the last wave of fr_ransac_kernel / of pnp_solve_kernel's first phase, thread 0 of pnp_finish_kernel): first-best-wins,
// adaptive iteration bound, stop at a failed sample -- so that evaluating all hypotheses
// concurrently gives exactly the serial algorithm's answer.  MPI = models per iteration slot
// (nmodels[it] in -1 (sampling failed) .. MPI, counts[it * MPI + k]).
template <int MPI>
__device__ inline RansacState ransac_replay(const RansacState *st_in, int first, int it_end, int max_iters, int n,
                                            double confidence, const int *__restrict__ nmodels,
                                            const int *__restrict__ counts, int model_points)
{
    RansacState s;
    if (first) {
        s.niters = max_iters;
        s.next_iter = 0;
        s.best_iter = -1;
        s.best_model = 0;
        s.best_count = 0;
        s.done = 0;
        s.iters_run = 0;
        s.pad = 0;
    } else {
        s = *st_in;
        if (s.done)
            return s;
    }
    int it = s.next_iter;
    if (n < model_points) {
        s.done = 1;
    } else {
        for (; it < it_end; it++) {
            if (it >= s.niters) {
                s.done = 1;
                break;
            }
            const int nm = nmodels[it];
            if (nm < 0) {
                s.done = 1;
                break;
            }
            for (int k = 0; k < nm; k++) {
                const int c = counts[it * MPI + k];
                const int floor_cnt = s.best_count > model_points - 1 ? s.best_count : model_points - 1;
                if (c > floor_cnt) {
                    s.best_count = c;
                    s.best_iter = it;
                    s.best_model = k;
                    s.niters = update_num_iters(confidence, (double)(n - c) / n, model_points, s.niters);
                }
            }
        }
        if (it >= s.niters || it >= max_iters)
            s.done = 1;
    }
    s.next_iter = it;
    s.iters_run = it;
    return s;
}

}  // namespace svo
