// removeDuplicates (include/monoUtils.h:195-213) through both adaptors, on a hand-made set.  No arguments.  Checks, and fails with a
// message when one does not hold:
//   * a new point on a base point, one at distance 10 (offset (6, 8): norm == radius, no duplicate), the next float inwards (a
//     duplicate), one far away;
//   * only the base points listed in `mask` take part; the list may repeat, be out of order and name points that do not exist;
//   * an EMPTY mask keeps everything (upstream's loop over it never runs) -- it must not turn into "all base points";
//   * the radius argument, its default of 10 and a negative radius (keeps everything);
//   * visualOdometry's member gives what visualSLAM's gives.
// Prints "replenish smoke ok" at the end.
#include <cmath>
#include <cstdio>
#include <vector>

#include "svo_compat/bundleAdjust.hpp"
#include "svo_compat/visualSLAM.hpp"

using namespace svo_compat;

#define FAIL(...)                          \
    do {                                   \
        std::fprintf(stderr, __VA_ARGS__); \
        std::fprintf(stderr, "\n");        \
        return 1;                          \
    } while (0)

static bool same(const std::vector<int> &got, std::initializer_list<int> want)
{
    return got == std::vector<int>(want);
}

static void show(const char *name, const std::vector<int> &v)
{
    std::printf("# %s", name);
    for (int i : v)
        std::printf(" %d", i);
    std::printf("\n");
}

int main()
{
    std::vector<Point2f> base, fresh;
    base.emplace_back(100.f, 100.f);   // 0
    base.emplace_back(300.f, 50.f);    // 1
    base.emplace_back(20.f, 200.f);    // 2
    fresh.emplace_back(100.f, 100.f);                          // 0: on base 0
    fresh.emplace_back(106.f, 108.f);                          // 1: norm == 10, not below it
    fresh.emplace_back(std::nextafter(106.f, 0.f), 108.f);     // 2: the next float inwards
    fresh.emplace_back(500.f, 400.f);                          // 3: far from everything
    fresh.emplace_back(304.f, 53.f);                           // 4: 5 from base 1
    fresh.emplace_back(20.f, 209.5f);                          // 5: 9.5 from base 2

    visualSLAM slam;
    visualOdometry vo;
    std::vector<int> all = {0, 1, 2}, none, odd = {2, 2, 7, -1, 0}, only1 = {1};
    std::vector<int> r;

    r = slam.removeDuplicates(base, fresh, all);   // radius 10 by default
    show("all", r);
    if (!same(r, {1, 3}))
        FAIL("all base points, radius 10: expected 1 3");
    r = slam.removeDuplicates(base, fresh, none);
    show("none", r);
    if (!same(r, {0, 1, 2, 3, 4, 5}))
        FAIL("an empty mask must keep every new point");
    r = slam.removeDuplicates(base, fresh, odd);   // base 2 twice, two entries outside the array, base 0
    show("odd", r);
    if (!same(r, {1, 3, 4}))
        FAIL("mask {2, 2, 7, -1, 0}: expected 1 3 4");
    r = slam.removeDuplicates(base, fresh, only1, 5);   // norm == 5 is not below 5
    show("only1", r);
    if (!same(r, {0, 1, 2, 3, 4, 5}))
        FAIL("mask {1}, radius 5: expected everything");
    r = slam.removeDuplicates(base, fresh, only1, 6);
    if (!same(r, {0, 1, 2, 3, 5}))
        FAIL("mask {1}, radius 6: expected 0 1 2 3 5");
    r = slam.removeDuplicates(base, fresh, all, -3);
    if (!same(r, {0, 1, 2, 3, 4, 5}))
        FAIL("a negative radius keeps everything");
    std::vector<Point2f> empty;
    if (!slam.removeDuplicates(base, empty, all).empty() || !same(slam.removeDuplicates(empty, fresh, none), {0, 1, 2, 3, 4, 5}))
        FAIL("empty sets");

    for (int radius : {0, 5, 10, 11})
        for (std::vector<int> *m : {&all, &none, &odd, &only1})
            if (vo.removeDuplicates(base, fresh, *m, radius) != slam.removeDuplicates(base, fresh, *m, radius))
                FAIL("visualOdometry::removeDuplicates differs from visualSLAM's at radius %d", radius);
    if (vo.removeDuplicates(base, fresh, all) != slam.removeDuplicates(base, fresh, all))
        FAIL("the default radius differs between the classes");
    std::printf("replenish smoke ok\n");
    return 0;
}
