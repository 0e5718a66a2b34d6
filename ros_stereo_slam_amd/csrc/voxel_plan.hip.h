// voxel_plan.hip.h -- the host decisions of voxel.hip (svo_voxel_downsample, svo_voxel_grid) with nothing of the HIP runtime in
// them: the argument refusals, the grid of a cloud's finite bounds and the capacity refusal decided from it, the cell of a
// coordinate, the key packing, the launch geometry and the layout of the work buffers.  voxel.hip includes it -- the key kernel
// forms its cells and keys with cell_index / pack_key below, so what runs on the device is what is checked here --; so does
// tests/cpp/voxel_plan_check.cpp, a stand-alone program that runs it under the address and undefined-behaviour sanitizers.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/svo.h"

#if defined(__HIPCC__)
#define VOXEL_PLAN_HD __host__ __device__
#else
#define VOXEL_PLAN_HD
#endif

namespace voxel_plan {

constexpr int MAX_POINTS = 1 << 22;         // the cap of svo_sor_filter_large, svo_cloud_create and the ICP
constexpr int AXIS_BITS = 21;               // bits of a cell index in the key
constexpr int64_t MAX_CELLS = 1ll << 21;    // an axis spanning this many cells or more is refused
constexpr int64_t CELLS_SATURATED = INT64_MAX;  // cells3 of an axis whose count does not fit
constexpr int BLOCK = 256;                  // threads of every tiled kernel
constexpr int TILE = 4096;                  // elements per workgroup: the radix sort's RS_TILE
constexpr int MEAN_WAVES = 4;               // voxels (one wavefront each) per workgroup of the accumulation
constexpr uint64_t DROPPED_KEY = ~0ull;     // a point with a non-finite coordinate: sorts behind every cell

// `v > 0 && v < inf` is false for a NaN
inline bool leaf_ok(double voxel_size) { return voxel_size > 0.0 && voxel_size < HUGE_VAL; }

// what svo_voxel_downsample refuses with SVO_ERR_ARG; 0, or the reason (the text svo_last_error returns)
inline const char *check_args(const void *ctx, const void *xyz, const void *color, int n, double voxel_size, const void *xyz_out,
                              const void *color_out, const void *n_out, int mem)
{
    if (!ctx)
        return "ctx must not be null";
    if (n < 0)
        return "n must not be negative";
    if (!leaf_ok(voxel_size))
        return "voxel_size must be positive and finite";
    if (mem != SVO_MEM_HOST && mem != SVO_MEM_DEVICE)
        return "mem must be SVO_MEM_HOST or SVO_MEM_DEVICE";
    if (n > 0 && (!xyz || !xyz_out || !n_out))
        return "xyz, xyz_out and n_out must not be null when n is not 0";
    if (n > 0 && color && !color_out)
        return "color_out must not be null when color is given";
    return nullptr;
}

// the cell of coordinate p on an axis whose grid starts at min_bound: a double subtraction, a double division, floor.  No
// reciprocal, no contraction (the library is built with -ffp-contract=off).  The caller has made sure the quotient fits.
VOXEL_PLAN_HD inline int64_t cell_index(float p, double min_bound, double voxel_size)
{
    return (int64_t)floor(((double)p - min_bound) / voxel_size);
}

// three cells of AXIS_BITS bits each, z the most significant: ascending keys are ascending (z, y, x)
VOXEL_PLAN_HD inline uint64_t pack_key(int64_t ix, int64_t iy, int64_t iz)
{
    return ((uint64_t)iz << (2 * AXIS_BITS)) | ((uint64_t)iy << AXIS_BITS) | (uint64_t)ix;
}

// svo_voxel_grid: min_bound3[a] = (double)min_xyz[a] - voxel_size * 0.5 and cells3[a] = the cell of max_xyz[a] + 1, the cells the
// axis spans (CELLS_SATURATED where that passes 2^62; compared in double first, so nothing overflows).  0 = fine; 1 = refused
// as an argument (*why set, nothing written): a null pointer, a bad leaf, a bound that is not finite, max below min;
// 2 = the outputs are written and an axis spans MAX_CELLS cells or more: what svo_voxel_downsample refuses with SVO_ERR_CAPACITY.
// Every point p of the cloud has min <= p <= max per axis, and the subtraction, the division by a positive leaf and floor are
// monotone: no cell index of the cloud exceeds cells3[a] - 1 <= 2^21 - 2.
inline int grid(const float *min_xyz, const float *max_xyz, double voxel_size, double *min_bound3, int64_t *cells3,
                const char **why)
{
    *why = nullptr;
    if (!min_xyz || !max_xyz || !min_bound3 || !cells3)
        return *why = "min_xyz, max_xyz, min_bound3 and cells3 must not be null", 1;
    if (!leaf_ok(voxel_size))
        return *why = "voxel_size must be positive and finite", 1;
    for (int a = 0; a < 3; a++)
        if (!std::isfinite(min_xyz[a]) || !std::isfinite(max_xyz[a]) || max_xyz[a] < min_xyz[a])
            return *why = "the bounds must be finite, max not below min", 1;
    int rc = 0;
    for (int a = 0; a < 3; a++) {
        min_bound3[a] = (double)min_xyz[a] - voxel_size * 0.5;
        const double q = floor(((double)max_xyz[a] - min_bound3[a]) / voxel_size);  // >= 0; may be huge or +inf
        cells3[a] = q < 4611686018427387904.0 /* 2^62 */ ? (int64_t)q + 1 : CELLS_SATURATED;
        if (cells3[a] >= MAX_CELLS) {
            *why = "voxel_size is too small: an axis of the cloud spans 2^21 cells or more";
            rc = 2;
        }
    }
    return rc;
}

inline int tiles(int n) { return (int)(((long long)n + TILE - 1) / TILE); }               // <= 1024 for n <= 2^22
inline int mean_blocks(int n) { return (int)(((long long)n + MEAN_WAVES - 1) / MEAN_WAVES); }

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// ctx->voxel_work of one call: n points, c floats a gathered row (3, or 6 with colours)
struct Layout {
    size_t k0, k1, v0, v1;  // the sort's keys and indices, and their ping-pong copies
    size_t hist;            // 256 x tiles(n) digit counts
    size_t rows;            // the finite points in voxel order: c floats a row
    size_t seg;             // n + 1 ints: the sorted position each voxel starts at, and the end of the last
    size_t part;            // tiles(n) x 8 words: a tile's lo x y z, hi x y z, finite count, pad
    size_t blk;             // tiles(n) ints: a tile's voxel heads, then their exclusive scan
    size_t scal;            // 8 words: the cloud's lo, hi and finite count; behind them n_out (word 8)
    size_t total;
};
inline Layout layout(int n, int c)
{
    Layout L;
    const size_t N = (size_t)n, T = (size_t)tiles(n);
    size_t off = 0;
    L.k0 = off, off = align256(off + N * 8);
    L.k1 = off, off = align256(off + N * 8);
    L.v0 = off, off = align256(off + N * 4);
    L.v1 = off, off = align256(off + N * 4);
    L.hist = off, off = align256(off + 256 * T * 4);
    L.rows = off, off = align256(off + N * (size_t)c * 4);
    L.seg = off, off = align256(off + (N + 1) * 4);
    L.part = off, off = align256(off + T * 32);
    L.blk = off, off = align256(off + T * 4);
    L.scal = off, off = align256(off + 64);
    L.total = off;
    return L;
}

// ctx->voxel_stage of a host call: both inputs, both outputs, the two trace arrays; n rows each
struct Stage {
    size_t xyz, color, xyz_out, color_out, point_voxel, voxel_count, total;
};
inline Stage stage(int n)
{
    Stage S;
    const size_t N = (size_t)n;
    size_t off = 0;
    S.xyz = off, off = align256(off + N * 12);
    S.color = off, off = align256(off + N * 12);
    S.xyz_out = off, off = align256(off + N * 12);
    S.color_out = off, off = align256(off + N * 12);
    S.point_voxel = off, off = align256(off + N * 4);
    S.voxel_count = off, off = align256(off + N * 4);
    S.total = off;
    return S;
}

}  // namespace voxel_plan
