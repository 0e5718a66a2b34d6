// gftt_plan_check.cpp -- the host arithmetic of csrc/gftt.hip (gftt_plan.hip.h: argument checks, cvRound and the cell grid, the keys of
// the maximum and of the sort, launch geometry, work-buffer layout) exercised on its own; tests/test_gftt_abi.py builds it with
// -fsanitize=address,undefined and runs it.  No GPU.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <limits>

#include "../../ros_stereo_slam_amd/csrc/gftt_plan.hip.h"

using namespace gftt_plan;

#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            return 1;                                                         \
        }                                                                     \
    } while (0)

static svo_gftt_params defaults()
{
    svo_gftt_params p = {1000, 3, 0, 0, 0.01, 1.0, 0.04};
    return p;
}

static int check_layout(const Plan &p, const svo_gftt_params &prm)
{
    const size_t offs[] = {p.off_max, p.off_base, p.off_counts, p.off_span, p.off_eig, p.off_mask, p.off_k0, p.off_k1, p.off_v0, p.off_v1,
                           p.off_hist, p.off_pxy, p.off_state, p.off_cell_start, p.off_cell_cursor, p.off_members, p.off_xy, p.off_resp,
                           p.total};
    for (size_t k = 0; k + 1 < sizeof(offs) / sizeof(offs[0]); k++) {
        EXPECT(offs[k] % 256 == 0);
        EXPECT(offs[k] <= offs[k + 1]);
    }
    EXPECT((long long)p.tiles_x * TILE_W >= p.w && (long long)(p.tiles_x - 1) * TILE_W < p.w);
    EXPECT((long long)p.tiles_y * TILE_H >= p.h && (long long)(p.tiles_y - 1) * TILE_H < p.h);
    const unsigned long long px = (unsigned long long)p.w * p.h;
    EXPECT((unsigned long long)p.spans * SPAN >= px && (unsigned long long)(p.spans - 1) * SPAN < px);
    EXPECT(p.groups * WAVES >= p.spans && (p.groups - 1) * WAVES < p.spans);
    EXPECT(px <= (1ull << 28) && (unsigned long long)p.spans * SPAN + SPAN < (1ull << 32));
    EXPECT(p.eig_lds <= 64 * 1024 && p.halo == 1 + prm.block_size / 2);
    EXPECT(p.max_cand <= (size_t)MAX_CANDIDATES);
    EXPECT(p.off_k1 - p.off_k0 >= p.max_cand * 8 && p.off_v1 - p.off_v0 >= p.max_cand * 4);
    EXPECT(p.off_pxy - p.off_hist >= 256 * ((p.max_cand + SORT_TILE - 1) / SORT_TILE) * 4);
    if (p.select) {
        EXPECT(p.cell >= 1 && p.cells == p.grid_w * p.grid_h);
        EXPECT((long long)p.grid_w * p.cell >= p.w && (long long)(p.grid_w - 1) * p.cell < p.w);
        EXPECT((long long)p.grid_h * p.cell >= p.h && (long long)(p.grid_h - 1) * p.cell < p.h);
        EXPECT(p.off_cell_cursor - p.off_cell_start >= (size_t)p.n_images * ((size_t)p.cells + 1) * 4);
    } else {
        EXPECT(p.cells == 0 && p.off_cell_cursor == p.off_cell_start);
    }
    return 0;
}

int main()
{
    svo_gftt_params prm = defaults();
    int n[16];
    float xy[2];
    const void *img = &prm;
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    // every refusal of svo.h, and the neighbours that pass
    EXPECT(check_args(img, &prm, xy, n, 1, 3, 3, 1, 1) == nullptr);
    EXPECT(check_args(img, &prm, xy, n, 1, 1, 1, 3, 1) == nullptr);
    EXPECT(check_args(img, &prm, xy, n, 16, 1026, 1026, 3, 1) == nullptr);      // 16 x 1024^2 = 2^24 interior pixels
    EXPECT(check_args(img, &prm, xy, n, 16, 1027, 1026, 3, 1));
    EXPECT(check_args(img, &prm, xy, n, 1, 4098, 4098, 1, 1) == nullptr);
    EXPECT(check_args(img, &prm, xy, n, 1, 16384, 16384, 1, 1));
    EXPECT(check_args(img, &prm, xy, n, 1, 16384, 2, 1, 1) == nullptr);         // no interior pixel: nothing to size
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
    for (int b = -3; b <= 40; b++) {
        svo_gftt_params q = defaults();
        q.block_size = b;
        EXPECT((check_params(&q) == nullptr) == (b >= 3 && b <= 31 && (b & 1)));
    }
    for (double q : {0.0, -0.1, 1.0000001, nan, inf}) {
        svo_gftt_params s = defaults();
        s.quality_level = q;
        EXPECT(check_params(&s));
    }
    for (double q : {1e-300, 0.01, 1.0}) {
        svo_gftt_params s = defaults();
        s.quality_level = q;
        EXPECT(check_params(&s) == nullptr);
    }
    for (double d : {-1e-9, -1.0, nan, -inf}) {
        svo_gftt_params s = defaults();
        s.min_distance = d;
        EXPECT(check_params(&s));
    }
    for (double d : {0.0, 0.4, 1.0, 1e9, inf}) {
        svo_gftt_params s = defaults();
        s.min_distance = d;
        EXPECT(check_params(&s) == nullptr);
    }
    for (double k : {nan, inf, 1e300}) {
        svo_gftt_params s = defaults();
        s.k = k;
        EXPECT(check_params(&s) == nullptr);   // k is not read without use_harris
        s.use_harris = 1;
        EXPECT(check_params(&s));
    }

    // cvRound: halves to even
    EXPECT(cv_round(0.5) == 0 && cv_round(1.5) == 2 && cv_round(2.5) == 2 && cv_round(3.5) == 4 && cv_round(1.0) == 1 &&
           cv_round(1.4999) == 1 && cv_round(32768.0) == 32768);

    // the keys: order, round trips, the fields of a sort key
    const float vals[] = {-std::numeric_limits<float>::infinity(), -3.5f, -1e-30f, -0.f, 0.f, 1e-38f, 1e-30f, 0.25f, 1.f,
                          3.4e38f};
    for (size_t a = 0; a < sizeof(vals) / sizeof(vals[0]); a++) {
        EXPECT(float_key(vals[a]) != 0);
        const float back = key_float(float_key(vals[a]));
        EXPECT(back == vals[a] && std::signbit(back) == std::signbit(vals[a]));
        if (a)
            EXPECT(float_key(vals[a - 1]) < float_key(vals[a]));
    }
    EXPECT(sort_key(0, 2.f, 5) < sort_key(0, 1.f, 5));          // value descending
    EXPECT(sort_key(0, 1.f, 6) < sort_key(0, 1.f, 5));          // index descending among equals
    EXPECT(sort_key(0, 1e-30f, 0) < sort_key(1, 3e38f, (1u << 28) - 1));   // image first
    for (int im : {0, 7, 15})
        for (float v : {1e-30f, 0.5f, -2.f})
            for (uint32_t idx : {0u, 1u, 12345u, (1u << 28) - 1}) {
                const uint64_t k = sort_key(im, v, idx);
                EXPECT(key_image(k) == im && key_value(k) == v && key_index(k) == idx);
            }
    EXPECT(quality_cut(2.f, 0.01) == (float)(2.0 * 0.01) && quality_cut(0.f, 0.5) == 0.f);

    // the layout at the sizes where the arithmetic could go wrong
    const int dims[] = {1, 2, 3, 7, 63, 64, 65, 1023, 1024, 1025, 1241, 4098, 16384};
    for (int w : dims)
        for (int h : dims)
            for (int ni : {1, 16}) {
                if (check_size(w, h, 1, ni))
                    continue;
                for (int b : {3, 5, 31})
                    for (double md : {0.0, 0.4, 1.0, 1.5, 2.5, 10.0, 1e9, inf})
                        for (int mode = 0; mode < 8; mode++) {
                            svo_gftt_params q = defaults();
                            q.block_size = b;
                            q.min_distance = md;
                            const Plan p = make_plan(w, h, mode & 1 ? 3 : 1, ni, 1000, &q, mode & 2, mode & 4, mode & 1);
                            if (check_layout(p, q))
                                return 1;
                            EXPECT(p.select == ((mode & 2) && md >= 1.0));
                            if (p.select && md == 2.5)
                                EXPECT(p.cell == 2);
                            if (p.select && md > 1e8)
                                EXPECT(p.cell == 32768 && p.cells == 1);
                        }
            }
    std::puts("gftt plan check ok");
    return 0;
}
