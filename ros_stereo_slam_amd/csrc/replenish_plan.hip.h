// replenish_plan.hip.h -- the host arithmetic of replenish.hip with nothing of HIP in it: the refusals of the two entry points, the
// capacity bound of svo_replenish and the geometry of the launches.  replenish.hip includes it; so does
// tests/cpp/replenish_plan_check.cpp, a stand-alone program that runs it under the address and undefined-behaviour sanitizers.
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/svo.h"

namespace replenish_plan {

constexpr int BLOCK = 256;      // duplicate test: one new point per lane
constexpr int TILE = 1024;      // reference points staged in LDS at a time (8 KiB)
constexpr int SEGMENTS = 16;    // append: as many single-wave workgroups as svo_compact uses
// n_ref, n_idx, n_new: every index the kernels form (a point, its third float, the end of a tile or of a segment) fits 32 bits
constexpr int MAX_POINTS = 1 << 28;

// what both entry points refuse about the duplicate test; 0, or the reason (the text svo_last_error returns).  `radius >= 0` is
// false for a NaN.
inline const char *check_common(const void *ctx, int n_ref, int n_new, double radius, int mode, int mem)
{
    if (!ctx)
        return "ctx must not be null";
    if (n_ref < 0 || n_new < 0)
        return "counts must not be negative";
    if (n_ref > MAX_POINTS || n_new > MAX_POINTS)
        return "at most 2^28 points a set";
    if (!(radius >= 0.0))
        return "radius must not be negative or NaN";
    if (mode != SVO_DEDUP_BOX && mode != SVO_DEDUP_DISC)
        return "mode must be SVO_DEDUP_BOX or SVO_DEDUP_DISC";
    if (mem != SVO_MEM_HOST && mem != SVO_MEM_DEVICE)
        return "mem must be SVO_MEM_HOST or SVO_MEM_DEVICE";
    return nullptr;
}

inline const char *check_dedup(const void *ctx, const void *ref_xy, int n_ref, const void *ref_idx, int n_idx, const void *new_xy,
                               int n_new, double radius, int mode, const void *keep, int mem)
{
    if (const char *why = check_common(ctx, n_ref, n_new, radius, mode, mem))
        return why;
    if (n_idx < 0)
        return "counts must not be negative";
    if (n_idx > MAX_POINTS)
        return "at most 2^28 points a set";
    if (n_idx != 0 && !ref_idx)
        return "ref_idx must not be null when n_idx is not 0";
    if (n_ref > 0 && !ref_xy)
        return "ref_xy must not be null when n_ref is not 0";
    if (n_new > 0 && (!new_xy || !keep))
        return "new_xy and keep must not be null when n_new is not 0";
    return nullptr;
}

// reference points the duplicate test walks: the listed ones, or all of them without a list
inline int sources(int n_ref, const void *ref_idx, int n_idx) { return ref_idx ? n_idx : n_ref; }

// Trip count of the tile loop, from the number of walked reference points ALONE: every wave of every workgroup runs the same
// number of tiles, whatever its lanes have found.
inline int tiles(int n_src) { return (int)(((long long)n_src + TILE - 1) / TILE); }

inline int blocks(int n_new) { return (int)(((long long)n_new + BLOCK - 1) / BLOCK); }

// svo_replenish: 0 = fine, 1 = a refusal with *why set (SVO_ERR_ARG), 2 = the worst case does not fit (SVO_ERR_CAPACITY).  The sum
// is formed in 64 bits: n_ref + n_new may pass 2^31.
inline int check_replenish(const void *ctx, const void *ref_xy, const void *ref_xyz, int n_ref, int cap, const void *new_xy,
                           const void *new_xyz, int n_new, double radius, int mode, const void *Rt, int mem, const char **why)
{
    if ((*why = check_common(ctx, n_ref, n_new, radius, mode, mem)))
        return 1;
    if (cap < 0)
        return *why = "counts must not be negative", 1;
    if (!Rt)
        return *why = "Rt must not be null", 1;
    if ((long long)cap < (long long)n_ref + (long long)n_new)
        return *why = "cap is below n_ref + n_new, the size when every new point is appended", 2;
    if (cap > 0 && (!ref_xy || !ref_xyz))
        return *why = "ref_xy and ref_xyz must not be null", 1;
    if (n_new > 0 && (!new_xy || !new_xyz))
        return *why = "new_xy and new_xyz must not be null when n_new is not 0", 1;
    return 0;
}

// append: every wavefront owns `seg` consecutive new points, whole 64-point strips; at most SEGMENTS wavefronts, at least one
inline int segment(int n_new)
{
    const long long per = ((long long)n_new + SEGMENTS - 1) / SEGMENTS;
    const long long seg = (per + 63) / 64 * 64;
    return (int)(seg > 0 ? seg : 64);
}
inline int segments(int n_new)
{
    const int seg = segment(n_new);
    const long long k = ((long long)n_new + seg - 1) / seg;
    return (int)(k > 0 ? k : 1);
}

}  // namespace replenish_plan
