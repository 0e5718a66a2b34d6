// fast_plan.hip.h -- the host arithmetic of fast.hip with nothing of HIP in it: the argument checks of the two entry points, the
// geometry of the launches, the layout of the work buffer and the cut of retainBest from a histogram.  fast.hip includes it; so does
// tests/cpp/fast_plan_check.cpp, a stand-alone program that runs it under the address and undefined-behaviour sanitizers.
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/svo.h"

#ifdef __HIPCC__
#define FAST_PLAN_HD __host__ __device__
#else
#define FAST_PLAN_HD
#endif

namespace fast_plan {

constexpr int MAX_DIM = 16384;   // w, h: a plane has at most 2^28 pixels, every index inside one plane fits 32 bits with room to spare
constexpr int MAX_BATCH = 16;
constexpr int BORDER = 3;        // radius of the ring
// score launch: a workgroup of 256 lanes owns TILE_W x TILE_H pixels, lane (t & 63, t >> 6) the rows ty, ty + 4, ...
constexpr int TILE_W = 64, TILE_H = 16;
// the staged tile: rows y0 - 3 ... y0 + TILE_H + 2, columns x0 - 4 ... x0 + TILE_W + 3 as whole dwords (x0 is a multiple of 64)
constexpr int LDS_ROWS = TILE_H + 2 * BORDER, LDS_DWORDS = (TILE_W + 8) / 4, LDS_PITCH = LDS_DWORDS * 4;
// suppress-and-compact: a wavefront owns SPAN consecutive pixels of the row-major plane, 64 at a time
constexpr int SPAN = 1024, WAVES = 4;

struct Plan {
    int w, h, c, n_images, cap;
    int pitch;             // bytes per row of the grey and of the fired planes, a multiple of 4
    int tiles_x, tiles_y;  // score launch: grid (tiles_x, tiles_y, n_images)
    int spans;             // wavefronts per image in the count / scatter launches: ceil(w h / SPAN), at most 2^18
    int groups;            // workgroups per image there: ceil(spans / WAVES)
    size_t plane_bytes;    // pitch * h
    // byte offsets into the work buffer, each a multiple of 256
    size_t off_counts, off_hist, off_cut, off_span_count, off_span_offset, off_fired, off_grey, off_xy, off_resp, off_score, off_idx,
        off_kept, off_oxy, off_oresp, total;
};

inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

// 0, or the reason the arguments are refused (the text svo_last_error returns)
inline const char *check_args(const void *images, const svo_fast_params *prm, const void *xy, const void *n, int n_images, int w, int h,
                              int c, int cap)
{
    if (!images || !prm || !xy || !n)
        return "images, prm, xy and n must not be null";
    if (c != 1 && c != 3)
        return "c must be 1 or 3";
    if (n_images < 1 || n_images > MAX_BATCH)
        return "n_images must be 1 ... 16";
    if (cap < 1)
        return "cap must be at least 1";
    if (w < 1 || h < 1 || w > MAX_DIM || h > MAX_DIM)
        return "w and h must be 1 ... 16384";
    if (prm->threshold < 0 || prm->threshold > 255)
        return "threshold must be 0 ... 255";
    if (prm->max_keypoints < 0)
        return "max_keypoints must not be negative";
    return nullptr;
}

// want_grey: the images are converted (c == 3) or copied (unaligned c == 1) into planes of the work buffer; want_score / host / anms:
// the staging the call needs beside the detector's own arrays
inline Plan make_plan(int w, int h, int c, int n_images, int cap, bool want_grey, bool want_score_stage, bool host, bool anms)
{
    Plan p{};
    p.w = w, p.h = h, p.c = c, p.n_images = n_images, p.cap = cap;
    p.pitch = (w + 3) & ~3;
    p.tiles_x = (w + TILE_W - 1) / TILE_W;
    p.tiles_y = (h + TILE_H - 1) / TILE_H;
    const size_t px = (size_t)w * (size_t)h;
    p.spans = (int)((px + SPAN - 1) / SPAN);
    p.groups = (p.spans + WAVES - 1) / WAVES;
    p.plane_bytes = (size_t)p.pitch * (size_t)h;
    const size_t ni = (size_t)n_images, e = ni * (size_t)cap;
    size_t o = 0;
    auto take = [&o](size_t bytes) {
        const size_t at = o;
        o += up256(bytes);
        return at;
    };
    p.off_counts = take(MAX_BATCH * sizeof(int));
    p.off_hist = take(ni * 256 * sizeof(int));
    p.off_cut = take(MAX_BATCH * sizeof(int));
    p.off_span_count = take(ni * (size_t)p.spans * sizeof(int));
    p.off_span_offset = take(ni * (size_t)p.spans * sizeof(int));
    p.off_fired = take(ni * p.plane_bytes);
    p.off_grey = take(want_grey ? ni * p.plane_bytes : 0);
    // the detector's lists: the caller's own arrays in device mode without ANMS, else these
    const bool lists = host || anms;
    p.off_xy = take(lists ? e * 8 : 0);
    p.off_resp = take(lists ? e * 4 : 0);
    p.off_score = take(want_score_stage ? ni * px : 0);
    p.off_idx = take(anms ? e * 4 : 0);
    p.off_kept = take(anms ? MAX_BATCH * sizeof(int) : 0);
    p.off_oxy = take(anms && host ? e * 8 : 0);
    p.off_oresp = take(anms && host ? e * 4 : 0);
    p.total = o;
    return p;
}

// KeyPointsFilter::retainBest on byte responses: hist[s] key points have response s.  The cut is the response of the
// max_keypoints-th best; every key point at or above it stays (ties included).  0 = everything stays.
FAST_PLAN_HD inline int retain_cut(const int *hist, int max_keypoints)
{
    long long total = 0;
    for (int s = 0; s < 256; s++)
        total += hist[s];
    if (max_keypoints <= 0 || total <= max_keypoints)
        return 0;
    long long above = 0;
    for (int s = 255; s > 0; s--) {
        above += hist[s];
        if (above >= max_keypoints)
            return s;
    }
    return 0;
}

}  // namespace fast_plan
