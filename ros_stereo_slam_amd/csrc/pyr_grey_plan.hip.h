// pyr_grey_plan.hip.h -- the address arithmetic of the two grey roles of pyramid.hip's base launch (a grey frame given as BGR is
// stored in one channel: level 0 is channel 0 of the raw image with its reflect-101 border, level 1 is filtered from channel 0 of
// the raw image), with nothing of the HIP runtime in it: which aligned dwords of the raw image a lane loads, how channel 0 is
// picked out of them, when an item may take that path (every loaded dword inside the image's 3 w h bytes) and how the level-0
// items are dealt over the workgroups of a grid that the host sized for three channels.  pyramid.hip includes it and its lanes
// call l0_group / l1_stage_item below, so what runs on the device is what is checked here; so does
// tests/cpp/pyr_grey_plan_check.cpp, a stand-alone program that replays every lane over buffers of exactly the image's size
// under the address and undefined-behaviour sanitizers.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define PYR_GREY_HD __host__ __device__ inline __attribute__((always_inline))
#define PYR_GREY_UNROLL _Pragma("unroll")
#else
#define PYR_GREY_HD inline
#define PYR_GREY_UNROLL
#endif

namespace pyr_grey_plan {

constexpr int PAD = 32;                       // SVO_PYR_PAD
constexpr int LANES = 64;                     // pyramid.hip's PB
constexpr int TILE_W = 32, TILE_H = 8;        // pyramid.hip's TW, TH: an output tile of level 1
constexpr int SRC_W = 2 * TILE_W + 3, SRC_H = 2 * TILE_H + 3;  // its staged source tile, 67 x 19 pixels
constexpr int SRC_ND = (SRC_W + 3) / 4;       // dwords of a staged row, 17: the last holds pixels 64, 65, 66 and 66 again
constexpr int GROUP = 16;                     // pixels of a level-0 item: one 16-byte store
constexpr int GROUP_RAW = 3 * (GROUP - 1) + 1;  // raw bytes from channel 0 of its first pixel to channel 0 of its last, 46

PYR_GREY_HD int reflect101(int p, int len)
{
    if (len == 1)
        return 0;
    while (p < 0 || p >= len)
        p = p < 0 ? -p : 2 * (len - 1) - p;
    return p;
}

// v_alignbyte_b32 and v_perm_b32, restated for the host: bytes sh .. sh + 3 of the eight bytes {lo: 0..3, hi: 4..7}; and the
// four bytes a selector names (0..3: lo, 4..7: hi, 0x0c: zero -- the selectors below use no other)
PYR_GREY_HD uint32_t alignbyte(uint32_t hi, uint32_t lo, unsigned sh)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbyte(hi, lo, sh);
#else
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * (sh & 3)));
#endif
}
PYR_GREY_HD uint32_t perm(uint32_t hi, uint32_t lo, uint32_t sel)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(hi, lo, sel);
#else
    const uint64_t both = ((uint64_t)hi << 32) | lo;
    uint32_t out = 0;
    for (int b = 0; b < 4; b++) {
        const unsigned s = (sel >> (8 * b)) & 0xff;
        out |= (s < 8 ? (uint32_t)((both >> (8 * s)) & 0xff) : 0u) << (8 * b);
    }
    return out;
#endif
}
// an aligned dword of the raw image (the host reads it with memcpy: the checker's buffers are byte arrays)
PYR_GREY_HD uint32_t load_dword(const uint8_t *p)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return *reinterpret_cast<const uint32_t *>(p);
#else
    uint32_t v;
    memcpy(&v, p, 4);
    return v;
#endif
}

// Channel 0 of four consecutive BGR pixels = raw bytes k, k + 3, k + 6, k + 9, where byte k is byte a (0..3) of q0 and q0..q3
// are consecutive aligned dwords (q3 is looked at only when a == 3: byte k + 9 is its first).  The three shifts bring bytes
// k .. k + 11 to n0 n1 n2, the selectors take bytes 0 and 3 of n0, 2 of n1, 1 of n2.
constexpr uint32_t SEL_0_3_6 = 0x0c060300u, SEL_KEEP3_9 = 0x05020100u;
// the staged row's last dword: pixels 64, 65, 66 and the spare byte, which repeats pixel 66 (what the edge path stages)
constexpr uint32_t SEL_0_3_6_6 = 0x06060300u;
PYR_GREY_HD uint32_t pick4(uint32_t q0, uint32_t q1, uint32_t q2, uint32_t q3, unsigned a)
{
    const uint32_t n0 = alignbyte(q1, q0, a), n1 = alignbyte(q2, q1, a), n2 = alignbyte(q3, q2, a);
    return perm(n2, perm(n1, n0, SEL_0_3_6), SEL_KEEP3_9);
}
PYR_GREY_HD uint32_t pick3_repeat(uint32_t q0, uint32_t q1, uint32_t q2, unsigned a)
{
    return perm(alignbyte(q2, q1, a), alignbyte(q1, q0, a), SEL_0_3_6_6);
}

// The aligned dwords a lane loads: n of them from byte `first` of the image on (a multiple of 4 as an ADDRESS; negative where
// the image starts inside the first dword), the wanted byte being byte a of the first.
struct Span {
    long long first;
    int n;
    unsigned a;
};
PYR_GREY_HD Span span_of(const uint8_t *img, long long s, int bytes)
{
    Span sp;
    sp.a = (unsigned)((reinterpret_cast<uintptr_t>(img) + (uintptr_t)s) & 3);
    sp.first = s - (long long)sp.a;
    sp.n = ((int)sp.a + bytes + 3) >> 2;
    return sp;
}
PYR_GREY_HD bool span_inside(const Span &sp, int w, int h) { return sp.first >= 0 && sp.first + 4ll * sp.n <= 3ll * w * h; }

// ------------------------------------------------------------------------------------------------ level 0
// An item is a group of GROUP pixels of a row of the padded grey level 0: group g of padded row `row` holds source pixels
// 16 g - PAD .. 16 g - PAD + 15 of source row reflect101(row - PAD, h); the pitch (svo_grey_pitch) is a multiple of 16.
PYR_GREY_HD int l0_pitch(int w) { return (w + 2 * PAD + 15) & ~15; }
PYR_GREY_HD int l0_groups(int w) { return l0_pitch(w) / GROUP; }
PYR_GREY_HD int l0_items(int w, int h) { return l0_groups(w) * (h + 2 * PAD); }
// no pixel of the group is reflected or lies in the pitch's slack
PYR_GREY_HD bool l0_interior(int w, int g) { return GROUP * g - PAD >= 0 && GROUP * g - PAD + GROUP <= w; }
// 12 dwords, or 13 where the 46 bytes start at byte 3 of the first
PYR_GREY_HD Span l0_span(const uint8_t *img, int w, int Y, int g)
{
    return span_of(img, 3ll * w * Y + 3ll * (GROUP * g - PAD), GROUP_RAW);
}
// the dword path: interior, and the tail guard -- no loaded dword in front of the image's first byte (the first group of row
// 0 of an image that is not dword-aligned) or behind its last (the last groups of the last row)
PYR_GREY_HD bool l0_dword_path(const uint8_t *img, int w, int h, int Y, int g)
{
    return l0_interior(w, g) && span_inside(l0_span(img, w, Y, g), w, h);
}
// the sixteen bytes of an item; true: by the dword path
PYR_GREY_HD bool l0_group(const uint8_t *img, int w, int h, int row, int g, uint32_t (&out)[4])
{
    const int Y = reflect101(row - PAD, h);
    if (l0_dword_path(img, w, h, Y, g)) {
        const Span sp = l0_span(img, w, Y, g);
        const uint8_t *p = img + sp.first;
        uint32_t q[13];
PYR_GREY_UNROLL
        for (int i = 0; i < 12; i++)
            q[i] = load_dword(p + 4 * i);
        q[12] = sp.n > 12 ? load_dword(p + 48) : 0u;
PYR_GREY_UNROLL
        for (int m = 0; m < 4; m++)
            out[m] = pick4(q[3 * m], q[3 * m + 1], q[3 * m + 2], q[3 * m + 3], sp.a);
        return true;
    }
    const uint8_t *srow = img + (size_t)Y * w * 3;
PYR_GREY_UNROLL
    for (int m = 0; m < 4; m++) {
        uint32_t v = 0;
PYR_GREY_UNROLL
        for (int b = 0; b < 4; b++) {
            const int px = GROUP * g + 4 * m + b;
            if (px < w + 2 * PAD)
                v |= (uint32_t)srow[reflect101(px - PAD, w) * 3] << (8 * b);
        }
        out[m] = v;
    }
    return false;
}
// The items row-major (item t: row t / groups, group t % groups), dealt in runs of l0_items_per_wg over the n_wg workgroups
// of the level-0 role -- a grid sized for three channels has about three workgroups where one channel filled one; the lanes
// of a workgroup take its run LANES apart.  Workgroups [ceil(items / per), n_wg) have none: the rounding remainder.
PYR_GREY_HD int l0_items_per_wg(int items, int n_wg) { return (items + n_wg - 1) / n_wg; }
PYR_GREY_HD void l0_run(int items, int n_wg, int wg, int *begin, int *end)
{
    const int per = l0_items_per_wg(items, n_wg);
    *begin = wg * per < items ? wg * per : items;
    *end = *begin + per < items ? *begin + per : items;
}

// ------------------------------------------------------------------------------------------------ level 1 from the raw image
// Tile (tx, ty) stages source pixels (x0 + i, y0 + r), x0 = 2 tx TILE_W - 2, y0 = 2 ty TILE_H - 2, i < 67, r < 19: an item
// is staged dword d of staged row r, pixels 4 d .. 4 d + 3 (d = 16: 64, 65, 66, 66).  Its raw bytes start at
PYR_GREY_HD long long l1_first_byte(int w, int x0, int y0, int r, int d) { return 3ll * w * (y0 + r) + 3ll * x0 + 12ll * d; }
// and it loads four dwords, whatever d and the alignment (no branch between a lane's loads: all turns' loads are in flight
// together); the last item of a row uses the first three
PYR_GREY_HD Span l1_span(const uint8_t *img, int w, int x0, int y0, int r, int d)
{
    Span sp = span_of(img, l1_first_byte(w, x0, y0, r, d), 0);
    sp.n = 4;
    return sp;
}
// the dword path: the tile's pixels lie inside the image, and the tail guard -- the dwords of the last item of the last row
// (the furthest any lane loads) end inside the buffer; the first item cannot start in front of it (x0 >= 62)
PYR_GREY_HD bool l1_tile_interior(const uint8_t *img, int w, int h, int x0, int y0)
{
    return x0 >= 0 && x0 + SRC_W <= w && y0 >= 0 && y0 + SRC_H <= h &&
           span_inside(l1_span(img, w, x0, y0, 0, 0), w, h) && span_inside(l1_span(img, w, x0, y0, SRC_H - 1, SRC_ND - 1), w, h);
}
PYR_GREY_HD uint32_t l1_stage_item(const uint8_t *img, int w, int x0, int y0, int r, int d)
{
    const Span sp = l1_span(img, w, x0, y0, r, d);
    const uint8_t *p = img + sp.first;
    const uint32_t q0 = load_dword(p), q1 = load_dword(p + 4), q2 = load_dword(p + 8), q3 = load_dword(p + 12);
    const uint32_t four = pick4(q0, q1, q2, q3, sp.a), last = pick3_repeat(q0, q1, q2, sp.a);
    return d == SRC_ND - 1 ? last : four;
}
constexpr int L1_ITEMS = SRC_H * SRC_ND;                       // 323 per tile
constexpr int L1_TURNS = (L1_ITEMS + LANES - 1) / LANES;       // lane `lane` takes items turn * LANES + lane

}  // namespace pyr_grey_plan
