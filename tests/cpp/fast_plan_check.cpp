// fast_plan_check.cpp -- the host arithmetic of csrc/fast.hip (fast_plan.hip.h: argument checks, launch geometry, work-buffer layout,
// retainBest's cut) exercised on its own; tests/test_fast_abi.py builds it with -fsanitize=address,undefined and runs it.  No GPU.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../ros_stereo_slam_amd/csrc/fast_plan.hip.h"

using namespace fast_plan;

#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            return 1;                                                         \
        }                                                                     \
    } while (0)

static int check_layout(const Plan &p)
{
    const size_t offs[] = {p.off_counts, p.off_hist, p.off_cut, p.off_span_count, p.off_span_offset, p.off_fired, p.off_grey, p.off_xy,
                           p.off_resp, p.off_score, p.off_idx, p.off_kept, p.off_oxy, p.off_oresp, p.total};
    for (size_t k = 0; k + 1 < sizeof(offs) / sizeof(offs[0]); k++) {
        EXPECT(offs[k] % 256 == 0);
        EXPECT(offs[k] <= offs[k + 1]);
    }
    EXPECT(p.pitch % 4 == 0 && p.pitch >= p.w && p.pitch < p.w + 4);
    EXPECT((long long)p.tiles_x * TILE_W >= p.w && (long long)(p.tiles_x - 1) * TILE_W < p.w);
    EXPECT((long long)p.tiles_y * TILE_H >= p.h && (long long)(p.tiles_y - 1) * TILE_H < p.h);
    const unsigned long long px = (unsigned long long)p.w * p.h;
    EXPECT((unsigned long long)p.spans * SPAN >= px && (unsigned long long)(p.spans - 1) * SPAN < px);
    EXPECT(p.groups * WAVES >= p.spans && (p.groups - 1) * WAVES < p.spans);
    // what the kernels index with 32 bits: a pixel of one plane, a dword of one plane, a wavefront's first pixel
    EXPECT(px <= (1ull << 28) && p.plane_bytes <= (1ull << 28) + 4ull * MAX_DIM);
    EXPECT((unsigned long long)p.spans * SPAN + SPAN < (1ull << 32));
    EXPECT(p.off_span_offset - p.off_span_count >= (size_t)p.n_images * p.spans * sizeof(int));
    EXPECT(p.off_grey - p.off_fired >= (size_t)p.n_images * p.plane_bytes);
    return 0;
}

int main()
{
    svo_fast_params prm = {10, 1, 0};
    int n[16];
    float xy[2];
    const void *img = &prm;
    // every refusal of svo.h, and the neighbours that pass
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
    for (int t : {-1, 256}) {
        svo_fast_params q = {t, 1, 0};
        EXPECT(check_args(img, &q, xy, n, 1, 7, 7, 1, 1));
    }
    svo_fast_params neg = {10, 1, -1};
    EXPECT(check_args(img, &neg, xy, n, 1, 7, 7, 1, 1));

    // the layout at the sizes where the arithmetic could go wrong: 1 x 1, the tile and span seams, the largest legal batch
    const int dims[] = {1, 3, 7, 63, 64, 65, 1023, 1024, 1025, 1241, 16383, 16384};
    for (int w : dims)
        for (int h : dims)
            for (int ni : {1, 16})
                for (int mode = 0; mode < 16; mode++) {
                    const size_t px = (size_t)w * h;
                    const int cap = (int)(px < 100000 ? px : 100000);
                    const Plan p = make_plan(w, h, mode & 1 ? 3 : 1, ni, cap, mode & 1, mode & 2, mode & 4, mode & 8);
                    if (check_layout(p))
                        return 1;
                    if (w == 16384 && h == 16384 && ni == 16)
                        EXPECT(p.total > (16ull << 28) && p.spans == (1 << 18));
                }

    // retainBest's cut against a sort
    std::vector<int> hist(256, 0);
    EXPECT(retain_cut(hist.data(), 5) == 0);
    unsigned s = 12345;
    for (int round = 0; round < 200; round++) {
        std::vector<int> resp;
        for (int &b : hist)
            b = 0;
        const int count = 1 + (int)((s = s * 1664525u + 1013904223u) >> 24);
        for (int k = 0; k < count; k++) {
            const int r = 1 + (int)((s = s * 1664525u + 1013904223u) >> 26) * (round % 4 + 1);   // 1 ... 253, many ties
            resp.push_back(r);
            hist[r]++;
        }
        for (int budget : {0, 1, 2, count / 2, count - 1, count, count + 1}) {
            const int cut = retain_cut(hist.data(), budget);
            std::vector<int> sorted(resp);
            for (size_t a = 0; a < sorted.size(); a++)   // insertion sort, descending
                for (size_t b = a; b > 0 && sorted[b] > sorted[b - 1]; b--) {
                    const int t = sorted[b];
                    sorted[b] = sorted[b - 1];
                    sorted[b - 1] = t;
                }
            const int want = budget <= 0 || count <= budget ? 0 : sorted[(size_t)budget - 1];
            EXPECT(cut == want);
        }
    }
    std::puts("fast plan check ok");
    return 0;
}
