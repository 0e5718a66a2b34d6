// star_plan.hip.h -- the host arithmetic of star.hip with nothing of HIP in it: the tables of the detector, the pattern count and
// border, the argument checks of the entry points, the overflow rule, the constants the response kernel takes, the geometry of the
// launches and the layout of the work buffer.  star.hip includes it; so does tests/cpp/star_plan_check.cpp, a stand-alone program
// that runs it under the address and undefined-behaviour sanitizers.
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/svo.h"

namespace star_plan {

constexpr int MAX_DIM = 16384;
constexpr int MAX_BATCH = 16;
constexpr int N_SIZES = 17, N_PAIRS = 12;
constexpr int SIZES0[N_SIZES] = {1, 2, 3, 4, 6, 8, 11, 12, 16, 22, 23, 32, 45, 46, 64, 90, 128};
// (outer index, inner index)
constexpr int PAIRS[N_PAIRS][2] = {{1, 0}, {3, 1}, {4, 2}, {5, 3}, {7, 4}, {8, 5}, {9, 6}, {11, 8}, {13, 10}, {14, 11}, {15, 12}, {16, 14}};
constexpr int MIN_KEYPOINT_SIZE = 4;
constexpr int WAVE = 64;   // tiles per wavefront of the tile and scatter launches = one entry of the scan

constexpr int tilt(int i) { return SIZES0[i] + SIZES0[i] / 2; }
// pixels of the square plus pixels of the diamond
constexpr int area(int i) { return (2 * SIZES0[i] + 1) * (2 * SIZES0[i] + 1) + tilt(i) * tilt(i) + (tilt(i) + 1) * (tilt(i) + 1); }

struct Layout {
    int npatterns, max_idx, border;
};

// the clamp at 12 is the library's: upstream's loop runs off its tables when max_size > 90
inline Layout layout(int w, int h, int max_size)
{
    const int m = w < h ? w : h;
    int n = 0;
    while (n < N_PAIRS && SIZES0[PAIRS[n][0]] < max_size && (n + 1 == N_PAIRS || tilt(PAIRS[n + 1][0]) < m))
        n++;
    Layout l;
    l.npatterns = n + 1 < N_PAIRS ? n + 1 : N_PAIRS;
    l.max_idx = PAIRS[l.npatterns - 1][0];
    l.border = tilt(l.max_idx);
    return l;
}

// how far from a key point of size sz the line test reads the planes, along x and along y
constexpr int line_reach(int sz) { return 4 * (sz / 4) + 1; }

// the largest entry of any of the three tables is at most 255 w h (integral_fits_int32's rule)
inline bool fits_int32(int w, int h) { return 255ll * w * h <= 2147483647ll; }

// what the response launch takes by value
struct Patterns {
    int npatterns, max_idx, border;
    unsigned need;   // bit i: the star sum of index i enters some pattern below npatterns
    float inv_inner[N_PAIRS], inv_outer[N_PAIRS];   // 1.f / innerArea, 1.f / outerArea: one IEEE division each, done here
};

inline Patterns make_patterns(const Layout &l)
{
    Patterns p{};
    p.npatterns = l.npatterns, p.max_idx = l.max_idx, p.border = l.border;
    for (int k = 0; k < N_PAIRS; k++) {
        const int o = PAIRS[k][0], i = PAIRS[k][1];
        p.inv_inner[k] = 1.f / (float)area(i);
        p.inv_outer[k] = 1.f / (float)(area(o) - area(i));
        if (k < l.npatterns)
            p.need |= (1u << o) | (1u << i);
    }
    return p;
}

inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

// 0, or the reason the parameters are refused
inline const char *check_params(const svo_star_params *prm)
{
    if (!prm)
        return "prm must not be null";
    if (prm->max_size < 3 || prm->max_size > 128)
        return "max_size must be 3 ... 128";
    if (prm->response_threshold < 0)
        return "response_threshold must not be negative";
    if (prm->line_threshold_projected < 0 || prm->line_threshold_binarized < 0)
        return "the line thresholds must not be negative";
    if (prm->suppress_nonmax_size < 1 || prm->suppress_nonmax_size > 31)
        return "suppress_nonmax_size must be 1 ... 31";
    return nullptr;
}

inline const char *check_image(int w, int h, int c)
{
    if (c != 1 && c != 3)
        return "c must be 1 or 3";
    if (w < 1 || h < 1 || w > MAX_DIM || h > MAX_DIM)
        return "w and h must be 1 ... 16384";
    return nullptr;
}

inline const char *check_args(const void *images, const svo_star_params *prm, const void *xy, const void *n, int n_images, int w, int h,
                              int c, int cap)
{
    if (!images || !xy || !n)
        return "images, xy and n must not be null";
    if (const char *why = check_params(prm))
        return why;
    if (const char *why = check_image(w, h, c))
        return why;
    if (n_images < 1 || n_images > MAX_BATCH)
        return "n_images must be 1 ... 16";
    if (cap < 1)
        return "cap must be at least 1";
    return nullptr;
}

struct Plan {
    int w, h, n_images, cap;
    Layout lay;
    bool empty;              // no pixel lies inside the border: the planes are zero and there is no key point
    int delta, step;         // suppress_nonmax_size / 2, the side of a tile
    int tiles_x, tiles_y;
    size_t tiles;            // per image
    size_t spans;            // wavefronts per image of the tile and scatter launches: ceil(tiles / 64)
    size_t table_stride;     // ints between the tables of two images: integral_img_stride
    // byte offsets into the work buffer, each a multiple of 256.  The three tables come first, the upright one at 0.
    size_t off_upright, off_even, off_odd, off_resp, off_size, off_tile, off_span_count, off_span_offset, off_counts, off_xy, off_ksize,
        off_kresp, total;
};

// host: the key-point columns are staged behind the detector's own arrays
inline Plan make_plan(int w, int h, int n_images, int cap, const svo_star_params *prm, bool host)
{
    Plan p{};
    p.w = w, p.h = h, p.n_images = n_images, p.cap = cap;
    p.lay = layout(w, h, prm->max_size);
    const int b = p.lay.border;
    p.empty = w <= 2 * b || h <= 2 * b;
    p.delta = prm->suppress_nonmax_size / 2;
    p.step = p.delta + 1;
    p.tiles_x = p.empty ? 0 : (w - 2 * b + p.step - 1) / p.step;
    p.tiles_y = p.empty ? 0 : (h - 2 * b + p.step - 1) / p.step;
    p.tiles = (size_t)p.tiles_x * (size_t)p.tiles_y;
    p.spans = (p.tiles + WAVE - 1) / WAVE;
    p.table_stride = (((size_t)(w + 1) * (size_t)(h + 1)) + 63) & ~(size_t)63;
    const size_t ni = (size_t)n_images, px = (size_t)w * (size_t)h, e = ni * (size_t)cap;
    size_t o = 0;
    auto take = [&o](size_t bytes) {
        const size_t at = o;
        o += up256(bytes);
        return at;
    };
    p.off_upright = take(ni * p.table_stride * 4);
    p.off_even = take(ni * p.table_stride * 4);
    p.off_odd = take(ni * p.table_stride * 4);
    p.off_resp = take(ni * px * 4);
    p.off_size = take(ni * px * 2);
    p.off_tile = take(ni * p.tiles * 4);
    p.off_span_count = take(ni * p.spans * 4);
    p.off_span_offset = take(ni * p.spans * 4);
    p.off_counts = take(MAX_BATCH * sizeof(int));
    p.off_xy = take(host ? e * 8 : 0);
    p.off_ksize = take(host ? e * 4 : 0);
    p.off_kresp = take(host ? e * 4 : 0);
    p.total = o;
    return p;
}

}  // namespace star_plan
