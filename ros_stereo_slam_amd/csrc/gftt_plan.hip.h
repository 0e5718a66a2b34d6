// gftt_plan.hip.h -- the host arithmetic of gftt.hip with nothing of HIP in it: the argument checks of the two entry points, cvRound
// and the cell grid of the minimum-distance selection, the order-preserving keys of the maximum and of the sort, the geometry of the
// launches and the layout of the work buffer.  gftt.hip includes it; so does tests/cpp/gftt_plan_check.cpp, a stand-alone program
// that runs it under the address and undefined-behaviour sanitizers.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../include/svo.h"

#ifdef __HIPCC__
#define GFTT_PLAN_HD __host__ __device__
#else
#define GFTT_PLAN_HD
#endif

namespace gftt_plan {

constexpr int MAX_DIM = 16384;   // w, h: a plane has at most 2^28 pixels, a row-major index fits the 28 low bits of a sort key
constexpr int MAX_BATCH = 16;    // the image index fits the 4 high bits of a sort key
// interior pixels, (w - 2)(h - 2), of all images of one call: what the candidate lists and the sort's arrays are sized to
constexpr long long MAX_CANDIDATES = 1ll << 24;
constexpr int MAX_BLOCK = 31;    // block_size: odd, 3 ... 31
constexpr double MAX_CELL = 32768.0;   // recipe G11: from a cell as large as the image on, the result does not depend on the cell
// eig launch: a workgroup of 256 lanes owns TILE_W x TILE_H pixels, lane (t & 63, t >> 6) the rows ty, ty + 4, ...
constexpr int TILE_W = 64;
constexpr int TILE_H = 16;
// candidate launches: a wavefront owns SPAN consecutive pixels of the row-major plane, 64 at a time
constexpr int SPAN = 1024;
constexpr int WAVES = 4;
constexpr int SORT_TILE = 4096;  // elements per workgroup of the radix sort (cloud_index.hip.h: RS_TILE)
constexpr int SELECT_T = 1024;   // threads of the selection's one workgroup per image

// cvRound: to nearest, halves to even (the default rounding mode)
inline int cv_round(double v) { return (int)std::nearbyint(v); }

// the float, as an unsigned that orders like it (-0 below +0); 0 is no float's key but a NaN's: "nothing seen"
GFTT_PLAN_HD inline uint32_t float_key(float f)
{
    uint32_t b;
    memcpy(&b, &f, 4);
    return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
GFTT_PLAN_HD inline float key_float(uint32_t k)
{
    const uint32_t b = k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu);
    float f;
    memcpy(&f, &b, 4);
    return f;
}
// ascending sort keys give: image ascending, value descending, row-major index descending (recipe G10)
GFTT_PLAN_HD inline uint64_t sort_key(int img, float v, uint32_t idx)
{
    return ((uint64_t)img << 60) | ((uint64_t)(~float_key(v)) << 28) | (uint64_t)(0x0fffffffu - idx);
}
GFTT_PLAN_HD inline int key_image(uint64_t k) { return (int)(k >> 60); }
GFTT_PLAN_HD inline float key_value(uint64_t k) { return key_float(~(uint32_t)(k >> 28)); }
GFTT_PLAN_HD inline uint32_t key_index(uint64_t k) { return 0x0fffffffu - (uint32_t)(k & 0x0fffffffu); }
// G7: the cut of threshold(TOZERO)
GFTT_PLAN_HD inline float quality_cut(float max_val, double quality_level) { return (float)((double)max_val * quality_level); }

struct Plan {
    int w, h, c, n_images, cap;
    int halo;              // 1 + block_size / 2: grey pixels staged around a tile
    int tiles_x, tiles_y;  // eig launch: grid (tiles_x, tiles_y, n_images)
    size_t eig_lds;        // its dynamic LDS bytes
    int spans;             // wavefronts per image in the candidate launches: ceil(w h / SPAN)
    int groups;            // workgroups per image there
    int select;            // min_distance >= 1: the selection rounds run
    int cell, grid_w, grid_h, cells;  // G11 (0 without selection)
    size_t max_cand;       // (w - 2)(h - 2) n_images
    // byte offsets into the work buffer, each a multiple of 256
    size_t off_max, off_base, off_counts, off_span, off_eig, off_mask, off_k0, off_k1, off_v0, off_v1, off_hist, off_pxy, off_state,
        off_cell_start, off_cell_cursor, off_members, off_xy, off_resp, total;
};

inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

// 0, or the reason the parameters are refused
inline const char *check_params(const svo_gftt_params *prm)
{
    if (prm->block_size < 3 || prm->block_size > MAX_BLOCK || !(prm->block_size & 1))
        return "block_size must be odd, 3 ... 31";
    if (!(prm->quality_level > 0.0) || !(prm->quality_level <= 1.0))
        return "quality_level must be in (0, 1]";
    if (!(prm->min_distance >= 0.0))
        return "min_distance must not be negative";
    if (prm->use_harris && !std::isfinite((float)prm->k))
        return "k must be finite as a float";
    return nullptr;
}

inline const char *check_size(int w, int h, int c, int n_images)
{
    if (c != 1 && c != 3)
        return "c must be 1 or 3";
    if (n_images < 1 || n_images > MAX_BATCH)
        return "n_images must be 1 ... 16";
    if (w < 1 || h < 1 || w > MAX_DIM || h > MAX_DIM)
        return "w and h must be 1 ... 16384";
    if (w >= 3 && h >= 3 && (long long)(w - 2) * (h - 2) * n_images > MAX_CANDIDATES)
        return "the images of one call must not have more than 2^24 interior pixels";
    return nullptr;
}

// 0, or the reason the arguments of svo_gftt_detect_batch are refused (the text svo_last_error returns)
inline const char *check_args(const void *images, const svo_gftt_params *prm, const void *xy, const void *n, int n_images, int w, int h,
                              int c, int cap)
{
    if (!images || !prm || !xy || !n)
        return "images, prm, xy and n must not be null";
    if (const char *why = check_size(w, h, c, n_images))
        return why;
    if (cap < 1)
        return "cap must be at least 1";
    return check_params(prm);
}

inline size_t eig_lds_bytes(int block_size)
{
    const int b = block_size / 2, r = b + 1;
    return (size_t)2 * (TILE_W + 2 * b) * (TILE_H + 2 * b) * sizeof(float) + (((size_t)(TILE_W + 2 * r) * (TILE_H + 2 * r) + 3) & ~(size_t)3);
}

// detect: the whole chain; otherwise svo_gftt_response's plane alone (stage_eig: a host caller's plane is staged)
inline Plan make_plan(int w, int h, int c, int n_images, int cap, const svo_gftt_params *prm, bool detect, bool host, bool masks)
{
    Plan p{};
    p.w = w, p.h = h, p.c = c, p.n_images = n_images, p.cap = cap;
    p.halo = 1 + prm->block_size / 2;
    p.tiles_x = (w + TILE_W - 1) / TILE_W;
    p.tiles_y = (h + TILE_H - 1) / TILE_H;
    p.eig_lds = eig_lds_bytes(prm->block_size);
    const size_t px = (size_t)w * (size_t)h, ni = (size_t)n_images;
    p.spans = (int)((px + SPAN - 1) / SPAN);
    p.groups = (p.spans + WAVES - 1) / WAVES;
    p.select = detect && prm->min_distance >= 1.0;
    if (p.select) {
        p.cell = cv_round(prm->min_distance < MAX_CELL ? prm->min_distance : MAX_CELL);
        p.grid_w = (w + p.cell - 1) / p.cell;
        p.grid_h = (h + p.cell - 1) / p.cell;
        p.cells = p.grid_w * p.grid_h;   // <= w h <= 2^28
    }
    p.max_cand = detect && w >= 3 && h >= 3 ? ni * (size_t)(w - 2) * (size_t)(h - 2) : 0;
    const size_t e = p.max_cand;
    size_t o = 0;
    auto take = [&o](size_t bytes) {
        const size_t at = o;
        o += up256(bytes);
        return at;
    };
    p.off_max = take(MAX_BATCH * sizeof(uint32_t));
    p.off_base = take((MAX_BATCH + 1) * sizeof(int));
    p.off_counts = take(MAX_BATCH * sizeof(int));
    p.off_span = take(detect ? (ni * (size_t)p.spans + 1) * sizeof(int) : 0);
    p.off_eig = take(detect || host ? ni * px * sizeof(float) : 0);
    p.off_mask = take(masks && host ? ni * px : 0);
    p.off_k0 = take(e * 8);
    p.off_k1 = take(e * 8);
    p.off_v0 = take(e * 4);
    p.off_v1 = take(e * 4);
    p.off_hist = take(e ? 256 * ((e + SORT_TILE - 1) / SORT_TILE) * sizeof(unsigned) : 0);
    p.off_pxy = take(e * 4);
    p.off_state = take(e * 4);
    p.off_cell_start = take(p.select ? ni * ((size_t)p.cells + 1) * sizeof(int) : 0);
    p.off_cell_cursor = take(p.select ? ni * (size_t)p.cells * sizeof(int) : 0);
    p.off_members = take(p.select ? e * 4 : 0);
    // the lists of a host call: cap entries an image, but no image has more corners than interior pixels
    p.off_xy = take(detect && host ? ni * (size_t)cap * 8 : 0);
    p.off_resp = take(detect && host ? ni * (size_t)cap * 4 : 0);
    p.total = o;
    return p;
}

}  // namespace gftt_plan
