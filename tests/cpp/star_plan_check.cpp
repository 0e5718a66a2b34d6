// star_plan_check.cpp -- the host arithmetic of csrc/star.hip (star_plan.hip.h: tables, pattern count, argument checks, overflow rule,
// launch geometry, work-buffer layout) exercised on its own; tests/test_star_abi.py builds it with -fsanitize=address,undefined and
// runs it.  No GPU.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "../../ros_stereo_slam_amd/csrc/star_plan.hip.h"

using namespace star_plan;

#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            return 1;                                                         \
        }                                                                     \
    } while (0)

static int check_plan(const Plan &p, const svo_star_params &prm, bool host)
{
    const size_t offs[] = {p.off_upright, p.off_even,    p.off_odd, p.off_resp,  p.off_size,  p.off_tile, p.off_span_count, p.off_span_offset,
                           p.off_counts,  p.off_xy,      p.off_ksize, p.off_kresp, p.total};
    for (size_t k = 0; k + 1 < sizeof(offs) / sizeof(offs[0]); k++) {
        EXPECT(offs[k] % 256 == 0);
        EXPECT(offs[k] <= offs[k + 1]);
    }
    const size_t ni = (size_t)p.n_images, px = (size_t)p.w * p.h, tab = (size_t)(p.w + 1) * (p.h + 1);
    EXPECT(p.off_upright == 0 && p.table_stride >= tab && p.table_stride < tab + 64 && p.table_stride % 64 == 0);
    EXPECT(p.off_even == ni * p.table_stride * 4 && p.off_odd - p.off_even >= ni * p.table_stride * 4);
    EXPECT(p.off_resp - p.off_odd >= ni * p.table_stride * 4);
    EXPECT(p.off_size - p.off_resp >= ni * px * 4 && p.off_tile - p.off_size >= ni * px * 2);
    EXPECT(p.off_span_count - p.off_tile >= ni * p.tiles * 4);
    EXPECT(p.off_span_offset - p.off_span_count >= ni * p.spans * 4 && p.off_counts - p.off_span_offset >= ni * p.spans * 4);
    EXPECT(p.off_xy - p.off_counts >= MAX_BATCH * sizeof(int));
    if (host) {
        const size_t e = ni * (size_t)p.cap;
        EXPECT(p.off_ksize - p.off_xy >= e * 8 && p.off_kresp - p.off_ksize >= e * 4 && p.total - p.off_kresp >= e * 4);
    } else {
        EXPECT(p.total == p.off_xy);
    }
    const int b = p.lay.border;
    EXPECT(p.delta == prm.suppress_nonmax_size / 2 && p.step == p.delta + 1 && p.step * p.step <= 256);   // a tile offset fits 8 bits
    EXPECT(p.empty == (p.w <= 2 * b || p.h <= 2 * b));
    if (p.empty) {
        EXPECT(p.tiles == 0 && p.spans == 0);
    } else {
        const long long iw = p.w - 2 * b, ih = p.h - 2 * b;
        EXPECT((long long)p.tiles_x * p.step >= iw && (long long)(p.tiles_x - 1) * p.step < iw);
        EXPECT((long long)p.tiles_y * p.step >= ih && (long long)(p.tiles_y - 1) * p.step < ih);
        EXPECT(p.tiles == (size_t)p.tiles_x * p.tiles_y && p.tiles <= (1ull << 28));
        EXPECT(p.spans * WAVE >= p.tiles && (p.spans - 1) * WAVE < p.tiles);
    }
    return 0;
}

int main()
{
    // the tables
    for (int i = 0; i + 1 < N_SIZES; i++)
        EXPECT(SIZES0[i] < SIZES0[i + 1]);
    for (int k = 0; k < N_PAIRS; k++) {
        EXPECT(PAIRS[k][0] > PAIRS[k][1] && PAIRS[k][0] < N_SIZES && PAIRS[k][1] >= 0);
        EXPECT(area(PAIRS[k][0]) > area(PAIRS[k][1]));
        EXPECT(k == 0 || (PAIRS[k][0] > PAIRS[k - 1][0] && PAIRS[k][1] > PAIRS[k - 1][1]));
    }
    for (int i = 0; i < N_SIZES; i++) {   // areas are pixel counts
        const int r = SIZES0[i], t = tilt(i);
        long long count = 0;
        for (int y = -t; y <= t; y++)
            for (int x = -t; x <= t; x++)
                count += (abs(x) <= r && abs(y) <= r) + (abs(x) + abs(y) <= t);
        EXPECT(count == area(i));
        // a star sum is at most 255 area: (float) of it and of an outer ring is exact or rounded once, never out of int range
        EXPECT(255ll * area(i) < (1ll << 31));
    }
    const Layout def = layout(1241, 376, 45);
    EXPECT(def.npatterns == 9 && def.max_idx == 13 && def.border == 69);

    // every accepted max_size at every image size that changes the count: the pattern count, the constants of the response launch,
    // and the proof that no sample of the line test leaves the image
    for (int max_size = 3; max_size <= 128; max_size++)
        for (int m = 1; m <= 400; m++) {
            const Layout l = layout(m, 16384, max_size);
            const Layout l2 = layout(16384, m, max_size);
            EXPECT(l.npatterns == l2.npatterns && l.max_idx == l2.max_idx && l.border == l2.border);
            EXPECT(l.npatterns >= 1 && l.npatterns <= N_PAIRS && l.max_idx == PAIRS[l.npatterns - 1][0] && l.border == tilt(l.max_idx));
            // upstream's loop, literally, wherever it stays inside its tables
            int n = 0;
            while (n < N_PAIRS && SIZES0[PAIRS[n][0]] < max_size && (n + 1 == N_PAIRS || tilt(PAIRS[n + 1][0]) < m))
                n++;
            EXPECT(l.npatterns == (n + 1 < N_PAIRS ? n + 1 : N_PAIRS));
            const Patterns pt = make_patterns(l);
            unsigned need = 0;
            for (int k = 0; k < l.npatterns; k++) {
                need |= (1u << PAIRS[k][0]) | (1u << PAIRS[k][1]);
                EXPECT(PAIRS[k][0] <= l.max_idx && tilt(PAIRS[k][0]) <= l.border);   // every read of the tables is inside them
                EXPECT(pt.inv_inner[k] == 1.f / (float)area(PAIRS[k][1]) && pt.inv_outer[k] == 1.f / (float)(area(PAIRS[k][0]) - area(PAIRS[k][1])));
                // a key point of this size lies at least `border` from every edge; the line test reads line_reach(sz) around it
                const int sz = SIZES0[PAIRS[k][0]];
                if (sz >= MIN_KEYPOINT_SIZE)
                    EXPECT(line_reach(sz) <= l.border);
            }
            EXPECT(pt.need == need && pt.npatterns == l.npatterns && pt.border == l.border);
        }

    // every refusal of svo.h, and the neighbours that pass
    svo_star_params prm = {45, 30, 10, 8, 5};
    int n[16];
    float xy[2];
    const void *img = &prm;
    EXPECT(check_args(img, &prm, xy, n, 1, 7, 7, 1, 1) == nullptr);
    EXPECT(check_args(img, &prm, xy, n, 16, 16384, 16384, 3, 1) == nullptr);
    EXPECT(check_args(img, &prm, xy, n, 1, 1, 1, 1, 1) == nullptr);
    EXPECT(check_args(nullptr, &prm, xy, n, 1, 7, 7, 1, 1));
    EXPECT(check_args(img, nullptr, xy, n, 1, 7, 7, 1, 1));
    EXPECT(check_args(img, &prm, nullptr, n, 1, 7, 7, 1, 1));
    EXPECT(check_args(img, &prm, xy, nullptr, 1, 7, 7, 1, 1));
    for (int c : {0, 2, 4, -1})
        EXPECT(check_args(img, &prm, xy, n, 1, 7, 7, c, 1));
    for (int k : {0, 17, -1})
        EXPECT(check_args(img, &prm, xy, n, k, 7, 7, 1, 1));
    for (int cap : {0, -5})
        EXPECT(check_args(img, &prm, xy, n, 1, 7, 7, 1, cap));
    for (int d : {0, -1, 16385, 1 << 30})
        EXPECT(check_args(img, &prm, xy, n, 1, d, 7, 1, 1) && check_args(img, &prm, xy, n, 1, 7, d, 1, 1));
    const svo_star_params bad[] = {{2, 30, 10, 8, 5}, {129, 30, 10, 8, 5}, {45, -1, 10, 8, 5}, {45, 30, -1, 8, 5},
                                   {45, 30, 10, -1, 5}, {45, 30, 10, 8, 0}, {45, 30, 10, 8, 32}, {-45, 30, 10, 8, 5}};
    for (const svo_star_params &q : bad)
        EXPECT(check_params(&q) && check_args(img, &q, xy, n, 1, 7, 7, 1, 1));
    const svo_star_params good[] = {{3, 0, 0, 0, 1}, {128, 2147483647, 2147483647, 2147483647, 31}};
    for (const svo_star_params &q : good)
        EXPECT(!check_params(&q));

    // the overflow rule: 255 w h <= 2^31 - 1
    EXPECT(fits_int32(2901, 2902) && fits_int32(1, 16384) && fits_int32(16384, 514));
    EXPECT(fits_int32(2048, 4112) && !fits_int32(2048, 4113) && !fits_int32(2902, 2902) && !fits_int32(16384, 16384));
    EXPECT(!fits_int32(16384, 515));

    // the layout at the sizes where the arithmetic could go wrong, up to the largest legal batch
    const int dims[] = {1, 6, 7, 13, 63, 64, 65, 138, 139, 140, 385, 1241, 16383, 16384};
    for (int w : dims)
        for (int h : dims)
            for (int ni : {1, 16})
                for (int host = 0; host < 2; host++)
                    for (int nonmax : {1, 2, 5, 31})
                        for (int max_size : {3, 4, 45, 128}) {
                            const svo_star_params q = {max_size, 30, 10, 8, nonmax};
                            const size_t px = (size_t)w * h;
                            const int cap = (int)(2 * px < 100000 ? 2 * px : 100000);
                            const Plan p = make_plan(w, h, ni, cap, &q, host);
                            if (check_plan(p, q, host))
                                return 1;
                            if (w == 16384 && h == 16384 && ni == 16 && nonmax == 1 && max_size == 3)
                                EXPECT(p.lay.border == 6 && p.total > (16ull << 28) * 21 && p.tiles == (size_t)(16384 - 12) * (16384 - 12));
                        }
    std::puts("star plan check ok");
    return 0;
}
