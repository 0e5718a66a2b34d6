// bm_plan.hip.h -- the host decisions of bm.hip (svo_bm_compute, svo_bm_prefilter) with nothing of the HIP runtime in them: the
// refusals, the band geometry (B3 of tests/bm_numpy.py), the tile of the matching kernel and its LDS layout against the budget,
// the cap on block_size and the layout of the context's scratch.  bm.hip includes it, so what is launched is what is checked
// here; so does tests/cpp/bm_plan_check.cpp, a stand-alone program that runs it under the address and undefined-behaviour
// sanitizers.
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/svo.h"

namespace bm_plan {

constexpr int MAX_W = 2048;                 // widest image: a column fits the 11 low bits of the validation key
constexpr int MAX_PAIRS = 16;
constexpr int MAX_D = 256;
constexpr int MIN_BLOCK = 5;
constexpr int MAX_BLOCK = 31;               // the cap on block_size (SVO_ERR_CAPACITY above it; the ABI allows up to 255)
constexpr int MAX_CAP = 63;
constexpr long long MAX_CELLS = 1ll << 30;  // pixel x disparity cells per call, refused from here on
constexpr int THREADS = 256;                // of the matching kernel
constexpr int BAND = 32;                    // rows a workgroup of the matching kernel produces
constexpr int TX_MAX = 64, TX_MIN = 8;      // band columns a workgroup produces: the largest power of two that fits
constexpr size_t LDS_BUDGET = 64 * 1024;    // per workgroup: what a launch gets without asking for more of a CU's 160 KB
constexpr size_t LDS_CU = 160 * 1024;
// a window's SAD (block^2 terms of at most 255) in 20 bits: the winner's key is sad * 512 + d in an int, the validation's
// key is cost << 11 | x in an unsigned
constexpr int MAX_SAD = MAX_BLOCK * MAX_BLOCK * 255;
static_assert(MAX_SAD < (1 << 20), "bm_match_kernel's and bm_validate_kernel's keys");
static_assert(MAX_W <= (1 << 11) && MAX_D <= 512, "bm_validate_kernel's and bm_match_kernel's keys");
static_assert(MAX_BLOCK * 255 < 65536, "the column sums are kept as uint16");
static_assert(MAX_BLOCK >= 31 && MAX_BLOCK % 2 == 1, "the issue's floor for the cap");

// 0 = fine, 1 = SVO_ERR_ARG, 2 = SVO_ERR_CAPACITY; *why: the reason.  Pointers, ctx and mem are the caller's to check.
inline int check(const svo_bm_params *p, int w, int h, int c, int n_pairs, const char **why)
{
    *why = nullptr;
    if (!p)
        return *why = "params must not be null", 1;
    if (n_pairs < 1 || n_pairs > MAX_PAIRS)
        return *why = "n_pairs must be 1..16", 1;
    if (c != 1 && c != 3)
        return *why = "c must be 1 or 3", 1;
    if (w < 1 || h < 1)
        return *why = "w and h must be positive", 1;
    if (p->num_disparities <= 0 || p->num_disparities % 16 != 0 || p->num_disparities > MAX_D)
        return *why = "num_disparities must be a positive multiple of 16 up to 256", 1;
    if (p->block_size % 2 == 0 || p->block_size < MIN_BLOCK || p->block_size > 255)
        return *why = "block_size must be odd and 5..255", 1;
    if (p->block_size > (w < h ? w : h))
        return *why = "block_size must not exceed min(w, h)", 1;
    if (p->pre_filter_cap < 1 || p->pre_filter_cap > MAX_CAP)
        return *why = "pre_filter_cap must be 1..63", 1;
    if (p->pre_filter_size % 2 == 0 || p->pre_filter_size < 5 || p->pre_filter_size > 255)
        return *why = "pre_filter_size must be odd and 5..255", 1;
    if (p->pre_filter_type != SVO_BM_PREFILTER_XSOBEL)
        return *why = "only SVO_BM_PREFILTER_XSOBEL is built", 1;
    if (p->texture_threshold < 0 || p->uniqueness_ratio < 0)
        return *why = "texture_threshold and uniqueness_ratio must not be negative", 1;
    // |minD| beyond this has an empty band at any legal width and would only overflow the geometry's ints
    if (p->min_disparity < -(1 << 20) || p->min_disparity > (1 << 20))
        return *why = "min_disparity must lie within +-2^20", 1;
    if (p->block_size > MAX_BLOCK)
        return *why = "block_size above the kernel's cap of 31", 2;
    if (w > MAX_W)
        return *why = "images wider than 2048 pixels", 2;
    if ((long long)w * h * n_pairs * p->num_disparities >= MAX_CELLS)
        return *why = "2^30 or more pixel x disparity cells per call", 2;
    return 0;
}

// B3.  xe: band columns that have a pixel (lofs + x < w); 0 when the band is empty
struct Geom {
    int lofs, rofs, width1, xe;
    bool empty;
};
inline Geom geometry(int w, int min_disparity, int num_disparities)
{
    Geom g;
    const int e = num_disparities - 1 + min_disparity;
    g.lofs = e > 0 ? e : 0;
    g.rofs = e < 0 ? -e : 0;
    g.width1 = w - g.rofs - num_disparities + 1;
    g.empty = g.lofs >= w || g.rofs >= w || g.width1 < 1;
    g.xe = g.empty ? 0 : (g.width1 < w - g.lofs ? g.width1 : w - g.lofs);
    return g;
}

inline size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }
inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// LDS of one workgroup of bm_match_kernel: a tile of tx band columns, D disparities, block = 2 r + 1.  ue: the tile with the
// window's margins; rw: the right strip (ue columns, D - 1 more for the disparities)
struct Lds {
    int tx, ue, rw, sad_stride;
    size_t colsum;   // uint16 [ue][D]: the vertical sums of the current row, kept running down the band
    size_t sad;      // int [tx][sad_stride]: the window sums of the current row
    size_t tcol;     // int [ue]: the vertical texture sums
    size_t rows;     // uint8: entering left [ue], leaving left [ue], entering right [rw], leaving right [rw]
    size_t total;
};
inline Lds lds(int tx, int D, int block)
{
    Lds L;
    L.tx = tx;
    L.ue = tx + block - 1;
    L.rw = L.ue + D - 1;
    L.sad_stride = D + THREADS / tx;   // the lanes of one column read THREADS / tx consecutive words: no two columns on one bank
    size_t off = 0;
    L.colsum = off, off = align16(off + (size_t)L.ue * D * 2);
    L.sad = off, off = align16(off + (size_t)tx * L.sad_stride * 4);
    L.tcol = off, off = align16(off + (size_t)L.ue * 4);
    L.rows = off, off = align16(off + 2 * (size_t)L.ue + 2 * (size_t)L.rw);
    L.total = off;
    return L;
}
// the tile: the largest of 64, 32, 16, 8 columns whose LDS stays inside the budget (8 always does: checked by the plan check)
inline int tile_width(int D, int block)
{
    int tx = TX_MAX;
    while (tx > TX_MIN && lds(tx, D, block).total > LDS_BUDGET)
        tx /= 2;
    return tx;
}

// ctx->bm_work of one call
struct Scratch {
    size_t pf;       // uint8 [2][n_pairs][h][w]: the pre-filtered left images, then the right ones
    size_t cost;     // int [n_pairs][h][w]: minsad per pixel, only with disp12_max_diff >= 0
    size_t parent;   // int [n_pairs][h][w] each: the speckle filter's union-find, only with a speckle window
    size_t sizes;
    size_t total;
};
inline Scratch scratch(int w, int h, int n_pairs, bool validate, bool speckle)
{
    Scratch S;
    const size_t npix = (size_t)w * h * n_pairs;
    size_t off = 0;
    S.pf = off, off = align256(off + 2 * npix);
    S.cost = off, off = align256(off + (validate ? npix * 4 : 0));
    S.parent = off, off = align256(off + (speckle ? npix * 4 : 0));
    S.sizes = off, off = align256(off + (speckle ? npix * 4 : 0));
    S.total = off;
    return S;
}

inline bool wants_validate(const svo_bm_params *p) { return p->disp12_max_diff >= 0; }
inline bool wants_speckle(const svo_bm_params *p) { return p->speckle_window_size > 0 && p->speckle_range >= 0; }

}  // namespace bm_plan
