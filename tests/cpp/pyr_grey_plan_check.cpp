// The address arithmetic of the grey roles of pyramid.hip's base launch (csrc/pyr_grey_plan.hip.h), replayed on the host: every
// lane of every workgroup of the level-0 role and of the level-1 role's interior tiles runs the header's own functions over a
// heap buffer of EXACTLY offset + 3 w h bytes with the image at buffer + offset, so that under -fsanitize=address,undefined a
// dword loaded in front of the image's allocation or behind its last byte ends the program.  What the lanes produce is compared
// with a plain byte-by-byte gather through reflect-101; the workgroup mapping has to hand out every item exactly once.
// One line per case: "case w h offset l0_items l0_dword l1_tiles l1_dword"; "pyr grey plan check ok" at the end.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../ros_stereo_slam_amd/csrc/pyr_grey_plan.hip.h"

namespace pgp = pyr_grey_plan;

static int fold(int p, int len)  // BORDER_REFLECT_101, written on its own
{
    if (len == 1)
        return 0;
    for (;;) {
        if (p < 0)
            p = -p;
        else if (p >= len)
            p = 2 * (len - 1) - p;
        else
            return p;
    }
}

#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            std::printf("FAILED %s: ", #cond);             \
            std::printf(__VA_ARGS__);                      \
            std::printf("\n");                             \
            std::exit(1);                                  \
        }                                                  \
    } while (0)

static void run_case(int w, int h, int offset)
{
    const size_t bytes = (size_t)3 * w * h;
    std::vector<uint8_t> *store = new std::vector<uint8_t>(offset + bytes);  // the allocation ends with the image
    uint8_t *buf = store->data();
    CHECK((reinterpret_cast<uintptr_t>(buf) & 15) == 0, "the allocator's alignment");
    uint32_t s = 12345u + 977u * w + 131u * h + offset;
    for (size_t i = 0; i < offset + bytes; i++) {  // noise, a stream of its own per byte: the channels differ
        s = s * 1664525u + 1013904223u;
        buf[i] = (uint8_t)(s >> 24);
    }
    const uint8_t *img = buf + offset;
    auto pixel = [&](int x, int y) { return img[((size_t)fold(y, h) * w + fold(x, w)) * 3]; };

    // ---- level 0: the grid of pyramid.hip's build_levels for three channels
    const int pitch3 = ((w + 2 * pgp::PAD) * 3 + 15) / 16 * 16;
    const int pad_x = (pitch3 / 4 + pgp::LANES - 1) / pgp::LANES, pad_y = (h + 2 * pgp::PAD + 7) / 8;
    const int n_wg = pad_x * pad_y, groups = pgp::l0_groups(w), items = pgp::l0_items(w, h);
    CHECK(pgp::l0_pitch(w) % 16 == 0 && pgp::l0_pitch(w) >= w + 2 * pgp::PAD && groups * (h + 2 * pgp::PAD) == items, "%d", w);
    std::vector<int> seen(items, 0);
    long l0_dword = 0;
    int empty = 0, first_empty = n_wg;
    for (int wg = 0; wg < n_wg; wg++) {
        int t0, t1;
        pgp::l0_run(items, n_wg, wg, &t0, &t1);
        CHECK(0 <= t0 && t0 <= t1 && t1 <= items, "wg %d: [%d, %d)", wg, t0, t1);
        if (t0 == t1) {
            empty++;
            first_empty = wg < first_empty ? wg : first_empty;
        }
        for (int lane = 0; lane < pgp::LANES; lane++)
            for (int t = t0 + lane; t < t1; t += pgp::LANES) {
                const int row = t / groups, g = t - row * groups;
                seen[t]++;
                uint32_t out[4] = {~0u, ~0u, ~0u, ~0u};
                l0_dword += pgp::l0_group(img, w, h, row, g, out) ? 1 : 0;
                for (int j = 0; j < pgp::GROUP; j++) {
                    const int px = pgp::GROUP * g + j;
                    const uint8_t want = px < w + 2 * pgp::PAD ? pixel(px - pgp::PAD, row - pgp::PAD) : 0;
                    const uint8_t got = (uint8_t)(out[j / 4] >> (8 * (j % 4)));
                    CHECK(got == want, "level 0 of %d x %d + %d: row %d pixel %d: %d, not %d", w, h, offset, row, px, got, want);
                }
            }
    }
    for (int t = 0; t < items; t++)
        CHECK(seen[t] == 1, "item %d of %d x %d handed out %d times", t, w, h, seen[t]);
    const int per = pgp::l0_items_per_wg(items, n_wg);
    CHECK(empty == n_wg - (items + per - 1) / per && first_empty == n_wg - empty, "%d of %d workgroups empty, the first is %d", empty,
          n_wg, first_empty);

    // ---- level 1 from the raw image: the interior tiles
    const int dw = (w + 1) / 2, dh = (h + 1) / 2;
    int l1_tiles = 0;
    long l1_dword = 0;
    for (int ty = 0; ty < (dh + pgp::TILE_H - 1) / pgp::TILE_H; ty++)
        for (int tx = 0; tx < (dw + pgp::TILE_W - 1) / pgp::TILE_W; tx++) {
            const int x0 = 2 * tx * pgp::TILE_W - 2, y0 = 2 * ty * pgp::TILE_H - 2;
            const bool geometric = x0 >= 0 && x0 + pgp::SRC_W <= w && y0 >= 0 && y0 + pgp::SRC_H <= h;
            const bool interior = pgp::l1_tile_interior(img, w, h, x0, y0);
            CHECK(!interior || geometric, "tile (%d, %d) of %d x %d", tx, ty, w, h);
            // only the tail guard may deny a tile that lies inside the image, and only on the image's last row
            CHECK(interior || !geometric || y0 + pgp::SRC_H == h, "tile (%d, %d) of %d x %d + %d denied", tx, ty, w, h, offset);
            if (!interior)
                continue;
            l1_tiles++;
            std::vector<int> staged(pgp::SRC_H * pgp::SRC_ND, 0);
            for (int lane = 0; lane < pgp::LANES; lane++)
                for (int turn = 0; turn < pgp::L1_TURNS; turn++) {
                    const int i = turn * pgp::LANES + lane;
                    if (i >= pgp::L1_ITEMS)
                        continue;
                    const int r = i / pgp::SRC_ND, d = i % pgp::SRC_ND;
                    staged[i]++;
                    const uint32_t v = pgp::l1_stage_item(img, w, x0, y0, r, d);
                    l1_dword++;
                    for (int bb = 0; bb < 4; bb++) {
                        const int px = 4 * d + bb < pgp::SRC_W - 1 ? 4 * d + bb : pgp::SRC_W - 1;  // the spare byte repeats the last
                        const uint8_t want = pixel(x0 + px, y0 + r), got = (uint8_t)(v >> (8 * bb));
                        CHECK(got == want, "tile (%d, %d) of %d x %d + %d: row %d byte %d: %d, not %d", tx, ty, w, h, offset, r, 4 * d + bb,
                              got, want);
                    }
                }
            for (int v : staged)
                CHECK(v == 1, "a staged dword written %d times", v);
        }
    std::printf("case %d %d %d %d %ld %d %ld\n", w, h, offset, items, l0_dword, l1_tiles, l1_dword);
    delete store;
}

int main()
{
    // the selectors, byte by byte
    CHECK(pgp::perm(0x77665544u, 0x33221100u, 0x07040300u) == 0x77443300u && pgp::perm(1u, 2u, 0x0c0c0c0cu) == 0u, "perm");
    CHECK(pgp::alignbyte(0x77665544u, 0x33221100u, 3) == 0x66554433u && pgp::alignbyte(7u, 0x33221100u, 0) == 0x33221100u, "alignbyte");
    const int ws[] = {44, 45, 46, 47, 128, 129, 130, 131, 132, 133, 135}, hs[] = {44, 45, 49, 51};
    for (int w : ws)
        for (int h : hs)
            for (int offset = 0; offset < 4; offset++)
                run_case(w, h, offset);
    for (int offset : {0, 3}) {
        run_case(260, 66, offset);
        run_case(516, 132, offset);
    }
    std::printf("pyr grey plan check ok\n");
    return 0;
}
