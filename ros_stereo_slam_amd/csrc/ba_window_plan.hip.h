// ba_window_plan.hip.h -- the host arithmetic of ba_window.hip with nothing of HIP in it: the refusals of svo_ba_window (the CSR
// validation included), the numbering of the free poses, the slab geometry and buffer sizes, the packed upper-triangle index and
// the Levenberg-Marquardt accept / reject rule, which the host applies once per trial and ba.hip's ba_3d2d_kernel on the device
// (the one piece marked for both under hipcc).  ba_window.hip and ba.hip include it; so does tests/cpp/ba_window_plan_check.cpp, a
// stand-alone program that runs it under the address and undefined-behaviour sanitizers.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/svo.h"

#if defined(__HIPCC__)  // as SVO_MATH_FN of include/svo_math.h
#define BA_PLAN_FN __host__ __device__ inline
#else
#define BA_PLAN_FN inline
#endif

namespace ba_window_plan {

constexpr int MAX_POSES = 32;   // poses of a window, fixed ones included: a point's run fits half a wavefront
constexpr int MAX_FREE = 16;    // free poses: the reduced system has at most 96 rows
constexpr int MAX_DIM = 6 * MAX_FREE;
constexpr int CHUNK = 32;       // points of one linearise + Schur workgroup (one wavefront) = one slab
constexpr int BLOCK = 256;      // threads of a back-substitution workgroup, one point each = one slab of two sums
constexpr int MAX_POINTS = 1 << 20;   // 32768 slabs of at most 38 KB
constexpr int MAX_OBS = 1 << 28;      // 3 * n_obs fits 32 bits

// packed upper triangle of a dim x dim symmetric matrix, row-major: (r, c) with r <= c
inline int tri_size(int dim) { return dim * (dim + 1) / 2; }
inline int tri_index(int dim, int r, int c) { return r * dim - r * (r - 1) / 2 + (c - r); }

// One slab of the linearise + Schur launch, in doubles: [ sum Hpl V^-1 Hpl^T (packed upper triangle) | sum Hpl V^-1 bl (dim) |
// Hpp (21 per free pose: the packed upper triangle of its 6 x 6 block) | bp (dim) | chi2 | max |diag Hll| ].  The sum of the
// slabs has the same layout.
struct SlabLayout {
    int dim, off_sb, off_hpp, off_bp, off_chi, off_max, stride;
};
inline SlabLayout slab_layout(int n_free)
{
    SlabLayout l;
    l.dim = 6 * n_free;
    l.off_sb = tri_size(l.dim);
    l.off_hpp = l.off_sb + l.dim;
    l.off_bp = l.off_hpp + 21 * n_free;
    l.off_chi = l.off_bp + l.dim;
    l.off_max = l.off_chi + 1;
    l.stride = (l.off_max + 1 + 7) & ~7;
    return l;
}
inline int schur_slabs(int n_points) { return (n_points + CHUNK - 1) / CHUNK; }
inline int backsub_slabs(int n_points) { return (n_points + BLOCK - 1) / BLOCK; }

struct Plan {
    int n_free = 0, n_obs = 0, n_stereo = 0;
    int free_index[MAX_POSES];   // pose -> row block of the reduced system, -1 for a held pose
    int free_list[MAX_FREE];     // row block -> pose, ascending
    int pose_obs[MAX_POSES];     // observations per pose
};

// What svo_ba_window refuses before it touches the device; 0, or the reason (the text svo_last_error returns).  obs_start, obs_pose
// and obs_uvr are HOST copies here whatever `mem` says.  The context is looked at last, so that every other refusal can be
// reached without a device.
inline const char *check_scalars(const svo_ba_window_params *p, int n_poses, const void *poses12, const uint8_t *pose_fixed,
                                 int n_points, const void *pts3d, const void *obs_start, const void *obs_pose, const void *obs_uvr,
                                 int mem, Plan *plan)
{
    if (!p || !poses12 || !pose_fixed || !pts3d || !obs_start || !obs_pose || !obs_uvr)
        return "null argument";
    if (mem != SVO_MEM_HOST && mem != SVO_MEM_DEVICE)
        return "mem must be SVO_MEM_HOST or SVO_MEM_DEVICE";
    if (n_poses < 1 || n_poses > MAX_POSES)
        return "n_poses must be 1..32";
    if (n_points < 1)
        return "n_points must be at least 1";
    if (n_points > MAX_POINTS)
        return "at most 2^20 points";
    if (p->iterations < 0)
        return "iterations must not be negative";
    if (!(p->huber_mono >= 0.0) || !(p->huber_stereo >= 0.0))
        return "a Huber delta must not be negative or NaN";
    plan->n_free = 0;
    for (int j = 0; j < n_poses; j++) {
        plan->pose_obs[j] = 0;
        if (pose_fixed[j]) {
            plan->free_index[j] = -1;
        } else {
            if (plan->n_free == MAX_FREE)
                return "more than 16 free poses";
            plan->free_index[j] = plan->n_free;
            plan->free_list[plan->n_free++] = j;
        }
    }
    if (plan->n_free == 0)
        return "no free pose";
    return nullptr;
}

inline const char *check_csr(const svo_ba_window_params *p, int n_poses, int n_points, const int *obs_start, const int *obs_pose,
                             const float *obs_uvr, Plan *plan)
{
    plan->n_obs = obs_start[n_points];
    plan->n_stereo = 0;
    for (int j = 0; j < n_poses; j++)
        plan->pose_obs[j] = 0;
    for (int i = 0; i < n_points; i++) {
        const int a = obs_start[i], b = obs_start[i + 1];
        uint32_t seen = 0;
        for (int o = a; o < b; o++) {
            const int j = obs_pose[o];
            if (j < 0 || j >= n_poses)
                return "obs_pose out of range";
            if (seen & (1u << j))
                return "a point seen twice by the same pose";
            seen |= 1u << j;
            plan->pose_obs[j]++;
            if (!std::isnan(obs_uvr[3 * (size_t)o + 2]))
                plan->n_stereo++;
        }
    }
    if (plan->n_stereo > 0 && !(p->bf > 0.0))
        return "a stereo observation needs bf > 0";
    for (int f = 0; f < plan->n_free; f++)
        if (plan->pose_obs[plan->free_list[f]] < 3)
            return "a free pose with fewer than three observations";
    return nullptr;
}

// obs_start alone (it sizes the copies of the other two arrays in device mode)
inline const char *check_starts(int n_points, const int *obs_start)
{
    if (obs_start[0] != 0)
        return "obs_start must begin at 0";
    for (int i = 0; i < n_points; i++) {
        if (obs_start[i + 1] < obs_start[i])
            return "obs_start must not decrease";
        if (obs_start[i + 1] > MAX_OBS)
            return "at most 2^28 observations";
    }
    return nullptr;
}

// ---- g2o's OptimizationAlgorithmLevenberg, one trial's decision: svo_ba_window's host loop and ba_3d2d_kernel ----------------------
struct LmState {
    double lambda = 0, ni = 2, chi = 0;   // chi: of the accepted estimate
    double rho = 0;
    int qmax = 0;
};
// computeLambdaInit: tau * max |diag H| over pose and point blocks
BA_PLAN_FN double lambda_init(double max_diag) { return 1e-5 * max_diag; }
// temp_chi / scale: the trial's chi2 and the sum dx (lambda dx + b) over every unknown; solved: the factorisation succeeded.
// Returns true when the trial is accepted.  The caller stops the trials of an iteration when !(rho < 0 && qmax < 10).
BA_PLAN_FN bool lm_trial(LmState &s, double temp_chi, double scale, bool solved)
{
    if (!solved)
        temp_chi = 1.7976931348623157e308;   // g2o: a failed solve is the largest chi2
    s.rho = (s.chi - temp_chi) / (scale + 1e-3);
    s.qmax++;
    if (s.rho > 0 && std::isfinite(temp_chi) && solved) {
        const double q = 2 * s.rho - 1;
        double alpha = 1. - q * q * q;
        alpha = std::fmin(alpha, 2. / 3.);
        s.lambda *= std::fmax(1. / 3., alpha);
        s.ni = 2;
        s.chi = temp_chi;
        return true;
    }
    s.lambda *= s.ni;
    s.ni *= 2;
    return false;
}

}  // namespace ba_window_plan
