// voxel_plan_check.cpp -- the host decisions of csrc/voxel.hip (voxel_plan.hip.h: the refusals, the grid and the capacity refusal,
// the cell of a coordinate, the key packing, the launch geometry, the buffer layouts) exercised on their own;
// tests/test_voxel_abi.py builds it with -fsanitize=address,undefined and runs it.  No GPU.
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "../../ros_stereo_slam_amd/csrc/voxel_plan.hip.h"

using namespace voxel_plan;

#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            return 1;                                                         \
        }                                                                     \
    } while (0)

int main()
{
    int token = 0;
    const void *p = &token;
    const double nan = std::nan(""), inf = HUGE_VAL;
    // svo_voxel_downsample: what passes, and every refusal of svo.h
    EXPECT(!check_args(p, p, p, 5, 0.1, p, p, p, SVO_MEM_HOST));
    EXPECT(!check_args(p, p, nullptr, 5, 1e-300, p, nullptr, p, SVO_MEM_DEVICE));
    EXPECT(!check_args(p, p, nullptr, 5, 1e300, p, p, p, SVO_MEM_HOST));               // color_out ignored without colours
    EXPECT(!check_args(p, nullptr, nullptr, 0, 0.1, nullptr, nullptr, nullptr, SVO_MEM_HOST));  // n == 0 needs no array
    EXPECT(!check_args(p, p, p, INT_MAX, 0.1, p, p, p, SVO_MEM_HOST));                 // the count's cap is SVO_ERR_CAPACITY, not this
    EXPECT(check_args(nullptr, p, p, 5, 0.1, p, p, p, SVO_MEM_HOST));
    EXPECT(check_args(p, p, p, -1, 0.1, p, p, p, SVO_MEM_HOST));
    EXPECT(check_args(p, p, p, INT_MIN, 0.1, p, p, p, SVO_MEM_HOST));
    for (double v : {0.0, -0.0, -1.0, -1e-300, nan, inf, -inf})
        EXPECT(check_args(p, p, p, 5, v, p, p, p, SVO_MEM_HOST) && !leaf_ok(v));
    for (int mem : {-1, 2, INT_MAX, INT_MIN})
        EXPECT(check_args(p, p, p, 5, 0.1, p, p, p, mem));
    EXPECT(check_args(p, nullptr, p, 5, 0.1, p, p, p, SVO_MEM_HOST));
    EXPECT(check_args(p, p, p, 5, 0.1, nullptr, p, p, SVO_MEM_HOST));
    EXPECT(check_args(p, p, p, 5, 0.1, p, p, nullptr, SVO_MEM_HOST));
    EXPECT(check_args(p, p, p, 5, 0.1, p, nullptr, p, SVO_MEM_HOST));

    // svo_voxel_grid: the minimum sits at reference coordinate 0.5, in cell 0
    const char *why = nullptr;
    double mb[3];
    int64_t cells[3];
    {
        const float lo[3] = {-1.f, 0.f, 2.f}, hi[3] = {1.f, 0.f, 2.5f};
        EXPECT(grid(lo, hi, 0.5, mb, cells, &why) == 0 && !why);
        EXPECT(mb[0] == -1.25 && mb[1] == -0.25 && mb[2] == 1.75);
        EXPECT(cells[0] == 5 && cells[1] == 1 && cells[2] == 2);
        for (int a = 0; a < 3; a++)
            EXPECT(((double)lo[a] - mb[a]) / 0.5 == 0.5 && cell_index(lo[a], mb[a], 0.5) == 0 &&
                   cell_index(hi[a], mb[a], 0.5) == cells[a] - 1);
    }
    // both sides of the 2^21 edge, leaf 1: the largest coordinate's cell is floor(max - min + 0.5)
    {
        const float lo[3] = {0.f, 0.f, 0.f};
        float hi[3] = {2097150.f, 0.f, 0.f};              // cell 2^21 - 2: 2^21 - 1 cells, accepted
        EXPECT(grid(lo, hi, 1.0, mb, cells, &why) == 0 && cells[0] == MAX_CELLS - 1);
        hi[0] = 2097151.f;                                // cell 2^21 - 1: 2^21 cells, refused
        EXPECT(grid(lo, hi, 1.0, mb, cells, &why) == 2 && cells[0] == MAX_CELLS && why && std::strstr(why, "too small"));
        EXPECT(mb[0] == -0.5 && cells[1] == 1 && cells[2] == 1);   // written also when refused
        hi[0] = 0.f, hi[2] = 2097151.f;                   // any axis
        EXPECT(grid(lo, hi, 1.0, mb, cells, &why) == 2 && cells[2] == MAX_CELLS);
        hi[2] = 2097150.f, hi[1] = 2097150.f;
        EXPECT(grid(lo, hi, 1.0, mb, cells, &why) == 0);
        // the largest accepted cells pack without touching a neighbour's bits
        const int64_t top = MAX_CELLS - 2;
        EXPECT(pack_key(top, top, top) == (((uint64_t)top << 42) | ((uint64_t)top << 21) | (uint64_t)top));
        EXPECT(pack_key(top, top, top) < DROPPED_KEY && pack_key(MAX_CELLS - 1, MAX_CELLS - 1, MAX_CELLS - 1) < (1ull << 63));
        EXPECT(pack_key(1, 0, 0) < pack_key(0, 1, 0) && pack_key(MAX_CELLS - 1, 0, 0) < pack_key(0, 1, 0) &&
               pack_key(MAX_CELLS - 1, MAX_CELLS - 1, 0) < pack_key(0, 0, 1));
    }
    // a quotient far beyond any integer: decided in double, nothing overflows
    {
        const float big = std::numeric_limits<float>::max();
        const float lo[3] = {-big, 0.f, 0.f}, hi[3] = {big, 0.f, 1.f};
        EXPECT(grid(lo, hi, 1e-300, mb, cells, &why) == 2 && cells[0] == CELLS_SATURATED && cells[1] == 1 && cells[2] == CELLS_SATURATED);
        EXPECT(grid(lo, hi, 1.0, mb, cells, &why) == 2 && cells[0] == CELLS_SATURATED && cells[2] == 2);
        EXPECT(grid(lo, hi, 1e300, mb, cells, &why) == 0 && cells[0] == 1);
        const float one[3] = {1.f, 1.f, 1.f};
        EXPECT(grid(one, one, 4.6e18, mb, cells, &why) == 0 && cells[0] == 1);
        const float l2[3] = {0.f, 0.f, 0.f}, h2[3] = {4.7e18f, 0.f, 0.f};   // q just above 2^62 at leaf 1
        EXPECT(grid(l2, h2, 1.0, mb, cells, &why) == 2 && cells[0] == CELLS_SATURATED);
        const float h3[3] = {4.5e18f, 0.f, 0.f};                            // just below: still an int64
        EXPECT(grid(l2, h3, 1.0, mb, cells, &why) == 2 && cells[0] > (1ll << 61) && cells[0] < CELLS_SATURATED);
    }
    // the argument refusals of svo_voxel_grid write nothing
    {
        const float lo[3] = {0.f, 0.f, 0.f}, hi[3] = {1.f, 1.f, 1.f};
        double m2[3] = {7, 7, 7};
        int64_t c2[3] = {7, 7, 7};
        EXPECT(grid(nullptr, hi, 1.0, m2, c2, &why) == 1 && why);
        EXPECT(grid(lo, nullptr, 1.0, m2, c2, &why) == 1);
        EXPECT(grid(lo, hi, 1.0, nullptr, c2, &why) == 1);
        EXPECT(grid(lo, hi, 1.0, m2, nullptr, &why) == 1);
        for (double v : {0.0, -1.0, nan, inf})
            EXPECT(grid(lo, hi, v, m2, c2, &why) == 1);
        const float bad[3] = {0.f, std::numeric_limits<float>::quiet_NaN(), 0.f}, binf[3] = {0.f, 0.f, std::numeric_limits<float>::infinity()};
        EXPECT(grid(bad, hi, 1.0, m2, c2, &why) == 1 && grid(lo, bad, 1.0, m2, c2, &why) == 1 && grid(lo, binf, 1.0, m2, c2, &why) == 1);
        EXPECT(grid(hi, lo, 1.0, m2, c2, &why) == 1);   // max below min
        for (int a = 0; a < 3; a++)
            EXPECT(m2[a] == 7 && c2[a] == 7);
    }
    // division, not a reciprocal: the kept case of tests/voxel_fixtures.py is searched there; here one known by hand --
    // 0.3 / 0.1 = 2.9999999999999996 in double, while 0.3 * (1 / 0.1) = 3.0000000000000004
    {
        const double num = 0.3, v = 0.1;
        EXPECT(floor(num / v) == 2.0 && floor(num * (1.0 / v)) == 3.0);
    }

    // launch geometry and layouts at the seams and at the cap: every region inside the total, aligned, in order
    for (int n : {1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8193, MAX_POINTS - 1, MAX_POINTS}) {
        const long long t = tiles(n), b = mean_blocks(n);
        EXPECT(t * TILE >= n && (t - 1) * TILE < n && t <= 1024);
        EXPECT(b * MEAN_WAVES >= n && (b - 1) * MEAN_WAVES < n);
        EXPECT(6LL * n <= INT_MAX && t * TILE <= INT_MAX);   // what the kernels form in 32 bits
        for (int c : {3, 6}) {
            const Layout L = layout(n, c);
            const size_t N = (size_t)n, offs[] = {L.k0, L.k1, L.v0, L.v1, L.hist, L.rows, L.seg, L.part, L.blk, L.scal, L.total};
            const size_t need[] = {N * 8, N * 8, N * 4, N * 4, (size_t)256 * t * 4, N * c * 4, (N + 1) * 4, (size_t)t * 32, (size_t)t * 4, 36};
            for (int k = 0; k < 10; k++)
                EXPECT(offs[k] % 256 == 0 && offs[k] + need[k] <= offs[k + 1]);
        }
        const Stage S = stage(n);
        const size_t N = (size_t)n, so[] = {S.xyz, S.color, S.xyz_out, S.color_out, S.point_voxel, S.voxel_count, S.total};
        const size_t sn[] = {N * 12, N * 12, N * 12, N * 12, N * 4, N * 4};
        for (int k = 0; k < 6; k++)
            EXPECT(so[k] % 256 == 0 && so[k] + sn[k] <= so[k + 1]);
    }
    std::puts("voxel plan check ok");
    return 0;
}
