// replenish_plan_check.cpp -- the host arithmetic of csrc/replenish.hip (replenish_plan.hip.h: the refusals, the capacity bound, the
// launch geometry) exercised on its own; tests/test_replenish_abi.py builds it with -fsanitize=address,undefined and runs it.  No GPU.
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "../../ros_stereo_slam_amd/csrc/replenish_plan.hip.h"

using namespace replenish_plan;

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
    const double nan = std::nan("");
    // svo_dedup_points: what passes, and every refusal of svo.h
    EXPECT(!check_dedup(p, p, 5, nullptr, 0, p, 7, 5.0, SVO_DEDUP_BOX, p, SVO_MEM_HOST));
    EXPECT(!check_dedup(p, p, 5, p, 3, p, 7, 0.0, SVO_DEDUP_DISC, p, SVO_MEM_DEVICE));
    EXPECT(!check_dedup(p, p, 5, p, 0, p, 7, 5.0, SVO_DEDUP_BOX, p, SVO_MEM_HOST));          // an empty list
    EXPECT(!check_dedup(p, nullptr, 0, nullptr, 0, nullptr, 0, 5.0, SVO_DEDUP_BOX, nullptr, SVO_MEM_HOST));
    EXPECT(!check_dedup(p, p, MAX_POINTS, p, MAX_POINTS, p, MAX_POINTS, HUGE_VAL, SVO_DEDUP_DISC, p, SVO_MEM_HOST));
    EXPECT(check_dedup(p, p, MAX_POINTS + 1, nullptr, 0, p, 7, 5.0, SVO_DEDUP_BOX, p, SVO_MEM_HOST));      // past 2^28 points
    EXPECT(check_dedup(p, p, 5, p, MAX_POINTS + 1, p, 7, 5.0, SVO_DEDUP_BOX, p, SVO_MEM_HOST));
    EXPECT(check_dedup(p, p, 5, nullptr, 0, p, INT_MAX, 5.0, SVO_DEDUP_BOX, p, SVO_MEM_HOST));
    EXPECT(check_dedup(nullptr, p, 5, nullptr, 0, p, 7, 5.0, SVO_DEDUP_BOX, p, SVO_MEM_HOST));
    EXPECT(check_dedup(p, p, -1, nullptr, 0, p, 7, 5.0, SVO_DEDUP_BOX, p, SVO_MEM_HOST));
    EXPECT(check_dedup(p, p, 5, p, -1, p, 7, 5.0, SVO_DEDUP_BOX, p, SVO_MEM_HOST));
    EXPECT(check_dedup(p, p, 5, nullptr, 0, p, -1, 5.0, SVO_DEDUP_BOX, p, SVO_MEM_HOST));
    EXPECT(check_dedup(p, p, 5, nullptr, 0, p, 7, -1e-300, SVO_DEDUP_BOX, p, SVO_MEM_HOST));
    EXPECT(check_dedup(p, p, 5, nullptr, 0, p, 7, nan, SVO_DEDUP_BOX, p, SVO_MEM_HOST));
    for (int mode : {-1, 2, INT_MAX, INT_MIN})
        EXPECT(check_dedup(p, p, 5, nullptr, 0, p, 7, 5.0, mode, p, SVO_MEM_HOST));
    for (int mem : {-1, 2})
        EXPECT(check_dedup(p, p, 5, nullptr, 0, p, 7, 5.0, SVO_DEDUP_BOX, p, mem));
    EXPECT(check_dedup(p, p, 5, nullptr, 3, p, 7, 5.0, SVO_DEDUP_BOX, p, SVO_MEM_HOST));     // n_idx != 0 without a list
    EXPECT(check_dedup(p, nullptr, 5, nullptr, 0, p, 7, 5.0, SVO_DEDUP_BOX, p, SVO_MEM_HOST));
    EXPECT(check_dedup(p, p, 5, nullptr, 0, nullptr, 7, 5.0, SVO_DEDUP_BOX, p, SVO_MEM_HOST));
    EXPECT(check_dedup(p, p, 5, nullptr, 0, p, 7, 5.0, SVO_DEDUP_BOX, nullptr, SVO_MEM_HOST));
    EXPECT(sources(5, nullptr, 0) == 5 && sources(5, p, 0) == 0 && sources(5, p, 9) == 9);

    // svo_replenish: the capacity bound is the worst case, formed without overflow
    const char *why = nullptr;
    EXPECT(check_replenish(p, p, p, 5, 12, p, p, 7, 5.0, SVO_DEDUP_BOX, p, SVO_MEM_HOST, &why) == 0);
    EXPECT(check_replenish(p, p, p, 5, 11, p, p, 7, 5.0, SVO_DEDUP_BOX, p, SVO_MEM_HOST, &why) == 2 && why && std::strstr(why, "cap"));
    EXPECT(check_replenish(p, p, p, MAX_POINTS, MAX_POINTS, p, p, 1, 5.0, SVO_DEDUP_BOX, p, SVO_MEM_HOST, &why) == 2);
    EXPECT(check_replenish(p, p, p, MAX_POINTS, INT_MAX, p, p, MAX_POINTS, 5.0, SVO_DEDUP_BOX, p, SVO_MEM_HOST, &why) == 0);
    EXPECT(check_replenish(p, p, p, MAX_POINTS, MAX_POINTS, p, p, 0, 5.0, SVO_DEDUP_BOX, p, SVO_MEM_HOST, &why) == 0);
    EXPECT(check_replenish(p, p, p, INT_MAX, INT_MAX, p, p, INT_MAX, 5.0, SVO_DEDUP_BOX, p, SVO_MEM_HOST, &why) == 1);
    EXPECT(check_replenish(p, nullptr, nullptr, 0, 0, nullptr, nullptr, 0, 5.0, SVO_DEDUP_DISC, p, SVO_MEM_DEVICE, &why) == 0);
    EXPECT(check_replenish(nullptr, p, p, 5, 12, p, p, 7, 5.0, SVO_DEDUP_BOX, p, SVO_MEM_HOST, &why) == 1);
    EXPECT(check_replenish(p, p, p, -1, 12, p, p, 7, 5.0, SVO_DEDUP_BOX, p, SVO_MEM_HOST, &why) == 1);
    EXPECT(check_replenish(p, p, p, 5, -1, p, p, 7, 5.0, SVO_DEDUP_BOX, p, SVO_MEM_HOST, &why) == 1);
    EXPECT(check_replenish(p, p, p, 5, 12, p, p, -1, 5.0, SVO_DEDUP_BOX, p, SVO_MEM_HOST, &why) == 1);
    EXPECT(check_replenish(p, p, p, 5, 12, p, p, 7, -1.0, SVO_DEDUP_BOX, p, SVO_MEM_HOST, &why) == 1);
    EXPECT(check_replenish(p, p, p, 5, 12, p, p, 7, nan, SVO_DEDUP_BOX, p, SVO_MEM_HOST, &why) == 1);
    EXPECT(check_replenish(p, p, p, 5, 12, p, p, 7, 5.0, 2, p, SVO_MEM_HOST, &why) == 1);
    EXPECT(check_replenish(p, p, p, 5, 12, p, p, 7, 5.0, SVO_DEDUP_BOX, p, 2, &why) == 1);
    EXPECT(check_replenish(p, p, p, 5, 12, p, p, 7, 5.0, SVO_DEDUP_BOX, nullptr, SVO_MEM_HOST, &why) == 1);
    EXPECT(check_replenish(p, nullptr, p, 5, 12, p, p, 7, 5.0, SVO_DEDUP_BOX, p, SVO_MEM_HOST, &why) == 1);
    EXPECT(check_replenish(p, p, nullptr, 5, 12, p, p, 7, 5.0, SVO_DEDUP_BOX, p, SVO_MEM_HOST, &why) == 1);
    EXPECT(check_replenish(p, p, p, 5, 12, nullptr, p, 7, 5.0, SVO_DEDUP_BOX, p, SVO_MEM_HOST, &why) == 1);
    EXPECT(check_replenish(p, p, p, 5, 12, p, nullptr, 7, 5.0, SVO_DEDUP_BOX, p, SVO_MEM_HOST, &why) == 1);

    // launch geometry at the seams and at the largest counts
    const int sizes[] = {0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 20000, 65536, MAX_POINTS - 1, MAX_POINTS};
    for (int n : sizes) {
        const long long t = tiles(n), b = blocks(n);
        EXPECT(t * TILE >= n && (t - 1) * TILE < n);
        EXPECT(b * BLOCK >= n && (b - 1) * BLOCK < n);
        const long long seg = segment(n), k = segments(n);
        EXPECT(seg >= 64 && seg % 64 == 0 && k >= 1 && k <= SEGMENTS);
        EXPECT(k * seg >= n && (n == 0 || (k - 1) * seg < n));
        EXPECT(k * seg <= INT_MAX && 3LL * n <= INT_MAX && t * TILE <= INT_MAX && b * BLOCK <= INT_MAX);   // what the kernels form in 32 bits
    }
    std::puts("replenish plan check ok");
    return 0;
}
