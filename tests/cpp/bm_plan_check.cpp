// The host decisions of csrc/bm.hip (bm_plan.hip.h) on their own, built with -fsanitize=address,undefined: every refusal, the band
// geometry against its definition, the tile and its LDS layout for every legal (D, block) -- regions in order, inside the
// budget, every index the kernel forms inside its region -- and the scratch layout at the corners of (w, h, n_pairs).  Prints the
// tile table ("tile D block tx lds") that tests/test_bm_abi.py compares with tests/bm_fixtures.py, then "bm plan check ok".
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "../../ros_stereo_slam_amd/csrc/bm_plan.hip.h"

#define REQUIRE(cond)                                                     \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::printf("%s:%d failed: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                     \
        }                                                                 \
    } while (0)

static svo_bm_params defaults()
{
    svo_bm_params p;
    p.pre_filter_type = SVO_BM_PREFILTER_XSOBEL;
    p.pre_filter_size = 9, p.pre_filter_cap = 31, p.block_size = 21, p.min_disparity = 0, p.num_disparities = 64;
    p.texture_threshold = 10, p.uniqueness_ratio = 15, p.speckle_window_size = 0, p.speckle_range = 0, p.disp12_max_diff = -1;
    return p;
}

static int rc_of(const svo_bm_params &p, int w, int h, int c, int n)
{
    const char *why = nullptr;
    const int rc = bm_plan::check(&p, w, h, c, n, &why);
    if ((rc != 0) != (why != nullptr))
        std::abort();
    return rc;
}

int main()
{
    using namespace bm_plan;
    const svo_bm_params d = defaults();
    const char *why = nullptr;
    REQUIRE(check(nullptr, 64, 64, 1, 1, &why) == 1 && why);
    REQUIRE(rc_of(d, 100, 50, 1, 1) == 0 && rc_of(d, 100, 50, 3, 16) == 0 && rc_of(d, 21, 21, 1, 1) == 0);
    // SVO_ERR_ARG
    for (int n : {0, -1, 17, INT_MAX, INT_MIN})
        REQUIRE(rc_of(d, 100, 50, 1, n) == 1);
    for (int c : {0, 2, 4, -1})
        REQUIRE(rc_of(d, 100, 50, c, 1) == 1);
    for (int nd : {0, -16, 8, 24, 272, 1024, INT_MAX, INT_MIN}) {
        svo_bm_params p = d;
        p.num_disparities = nd;
        REQUIRE(rc_of(p, 100, 50, 1, 1) == 1);
    }
    for (int b : {0, 1, 3, 4, 6, 20, 22, 256, 257, -5, INT_MAX, INT_MIN}) {
        svo_bm_params p = d;
        p.block_size = b;
        REQUIRE(rc_of(p, 600, 600, 1, 1) == 1);
    }
    REQUIRE(rc_of(d, 20, 50, 1, 1) == 1 && rc_of(d, 50, 20, 1, 1) == 1 && rc_of(d, 0, 50, 1, 1) == 1 && rc_of(d, 50, -1, 1, 1) == 1);
    for (int cap : {0, -1, 64, INT_MAX}) {
        svo_bm_params p = d;
        p.pre_filter_cap = cap;
        REQUIRE(rc_of(p, 100, 50, 1, 1) == 1);
    }
    for (int s : {0, 3, 4, 6, 10, 257, -9}) {
        svo_bm_params p = d;
        p.pre_filter_size = s;
        REQUIRE(rc_of(p, 100, 50, 1, 1) == 1);
    }
    for (int t : {(int)SVO_BM_PREFILTER_NORMALIZED_RESPONSE, 2, -1}) {
        svo_bm_params p = d;
        p.pre_filter_type = t;
        REQUIRE(rc_of(p, 100, 50, 1, 1) == 1);
    }
    {
        svo_bm_params p = d;
        p.texture_threshold = -1;
        REQUIRE(rc_of(p, 100, 50, 1, 1) == 1);
        p = d, p.uniqueness_ratio = -1;
        REQUIRE(rc_of(p, 100, 50, 1, 1) == 1);
        for (int m : {INT_MAX, INT_MIN, (1 << 20) + 1, -(1 << 20) - 1}) {
            p = d, p.min_disparity = m;
            REQUIRE(rc_of(p, 100, 50, 1, 1) == 1);
        }
    }
    // SVO_ERR_CAPACITY
    for (int b = MAX_BLOCK + 2; b <= 255; b += 2) {
        svo_bm_params p = d;
        p.block_size = b;
        REQUIRE(rc_of(p, 600, 600, 1, 1) == 2);
    }
    REQUIRE(rc_of(d, MAX_W + 1, 50, 1, 1) == 2 && rc_of(d, MAX_W, 50, 1, 1) == 0);
    {
        svo_bm_params p = d;
        p.num_disparities = 256;
        REQUIRE(rc_of(p, 2048, 128, 1, 16) == 2);    // 2^30 cells exactly
        REQUIRE(rc_of(p, 2048, 127, 1, 16) == 0);
        REQUIRE(rc_of(p, 2048, INT_MAX, 1, 16) == 2);
    }
    // geometry: against the definition, and the band inside the image
    for (int w : {1, 5, 16, 17, 100, 2048})
        for (int D = 16; D <= MAX_D; D += 16)
            for (int minD : {-(1 << 20), -3000, -300, -17, -16, -15, -3, 0, 1, 5, 100, 2047, 3000, 1 << 20}) {
                const Geom g = geometry(w, minD, D);
                const long long e = (long long)D - 1 + minD;
                REQUIRE(g.lofs == (e > 0 ? e : 0) && g.rofs == (e < 0 ? -e : 0) && g.width1 == w - g.rofs - D + 1);
                REQUIRE(g.empty == (g.lofs >= w || g.rofs >= w || g.width1 < 1));
                if (g.empty) {
                    REQUIRE(g.xe == 0);
                    continue;
                }
                REQUIRE(g.xe >= 1 && g.xe <= g.width1 && g.lofs + g.xe <= w);
                // the right strip's last column: rofs + width1 - 1 + D - 1 is the image's last
                REQUIRE(g.rofs + g.width1 - 1 + D - 1 == w - 1);
            }
    // the tile and its LDS for every legal (D, block)
    for (int D = 16; D <= MAX_D; D += 16)
        for (int block = MIN_BLOCK; block <= MAX_BLOCK; block += 2) {
            const int tx = tile_width(D, block);
            REQUIRE(tx >= TX_MIN && tx <= TX_MAX && (tx & (tx - 1)) == 0 && THREADS % tx == 0 && THREADS / tx <= 64);
            const Lds L = lds(tx, D, block);
            REQUIRE(L.total <= LDS_BUDGET && LDS_BUDGET <= LDS_CU);
            REQUIRE(tx == TX_MAX || lds(2 * tx, D, block).total > LDS_BUDGET);   // the largest that fits
            REQUIRE(L.ue == tx + block - 1 && L.rw == L.ue + D - 1 && L.sad_stride >= D);
            REQUIRE(L.colsum == 0 && L.colsum + (size_t)L.ue * D * 2 <= L.sad && L.sad % 4 == 0);
            REQUIRE(L.sad + (size_t)tx * L.sad_stride * 4 <= L.tcol && L.tcol % 4 == 0);
            REQUIRE(L.tcol + (size_t)L.ue * 4 <= L.rows && L.rows + 2 * (size_t)L.ue + 2 * (size_t)L.rw <= L.total);
            // the kernel's largest indices: colsum[(tx - 1 + 2r) * D + D - 1], the right strip's [ue - 1 + D - 1],
            // tcol[tx - 1 + 2r], the thread mapping of the horizontal sums
            const int r = block / 2;
            REQUIRE(tx - 1 + 2 * r == L.ue - 1 && L.ue - 1 + D - 1 == L.rw - 1 && L.ue <= THREADS);
            const int nseg = THREADS / D > 1 ? THREADS / D : 1, seglen = (tx + nseg - 1) / nseg;
            REQUIRE(nseg * D <= THREADS && nseg * seglen >= tx);
            std::printf("tile %d %d %d %zu\n", D, block, tx, L.total);
        }
    // scratch: regions in order, inside the total, at the corners
    for (int w : {5, 2048})
        for (int h : {5, 4096})
            for (int n : {1, 16})
                for (int v = 0; v < 2; v++)
                    for (int s = 0; s < 2; s++) {
                        const Scratch S = scratch(w, h, n, v, s);
                        const size_t npix = (size_t)w * h * n;
                        REQUIRE(S.pf == 0 && S.pf + 2 * npix <= S.cost && S.cost % 256 == 0);
                        REQUIRE(S.cost + (v ? npix * 4 : 0) <= S.parent && S.parent + (s ? npix * 4 : 0) <= S.sizes);
                        REQUIRE(S.sizes + (s ? npix * 4 : 0) <= S.total && S.total <= 2 * npix + 12 * npix + 4 * 256);
                    }
    svo_bm_params p = d;
    REQUIRE(!wants_validate(&p) && !wants_speckle(&p));
    p.disp12_max_diff = 0, p.speckle_window_size = 1;
    REQUIRE(wants_validate(&p) && wants_speckle(&p));
    p.speckle_range = -1;
    REQUIRE(!wants_speckle(&p));
    std::printf("bm plan check ok\n");
    return 0;
}
