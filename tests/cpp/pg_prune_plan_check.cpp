// pg_prune_plan_check.cpp -- the host arithmetic of the pose graph's pruning (csrc/pg_prune_plan.hip.h: the kernels that are refused,
// which edges go, the remap, the reachability test, the two refusals) exercised on its own; tests/test_pg_robust_abi.py builds it with
// -fsanitize=address,undefined and runs it.  No GPU.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../ros_stereo_slam_amd/csrc/pg_prune_plan.hip.h"

using namespace pg_prune_plan;

#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            return 1;                                                         \
        }                                                                     \
    } while (0)

int main()
{
    const double nan = std::nan(""), inf = std::numeric_limits<double>::infinity();
    const int GM = SVO_PG_ROBUST_GEMAN_MCCLURE, NONE = SVO_PG_ROBUST_NONE;
    // the kernels
    for (int kind = SVO_PG_ROBUST_HUBER; kind <= GM; kind++) {
        EXPECT(!check_kernel(kind, 1.0) && !check_kernel(kind, 1e-300) && !check_kernel(kind, 1e300));
        EXPECT(check_kernel(kind, 0.0) && check_kernel(kind, -1.0) && check_kernel(kind, nan) && check_kernel(kind, inf));
    }
    EXPECT(!check_kernel(NONE, 0.0) && !check_kernel(NONE, nan));
    EXPECT(check_kernel(-1, 1.0) && check_kernel(5, 1.0) && check_kernel(1 << 30, 1.0));

    Plan p;
    // empty graph, and a graph whose edges carry no kernel
    EXPECT(plan(1, 0, nullptr, nullptr, nullptr, nullptr, 0.25, 0, p) == PRUNE_OK && p.removed.empty() && p.remap.empty());
    {
        const int f[] = {0, 1, 2}, t[] = {1, 2, 0};
        const double w[] = {0, 0, 0};
        EXPECT(plan(3, 3, f, t, nullptr, w, 0.25, 0, p) == PRUNE_OK && p.removed.empty());
        EXPECT(p.remap == std::vector<int>({0, 1, 2}));
    }
    // a chain 0-1-2-3-4 with closures; the first and the last edge of the list are closures
    {
        const int f[] = {3, 0, 1, 2, 3, 4, 4}, t[] = {0, 1, 2, 3, 4, 1, 0};
        const int k[] = {GM, NONE, NONE, NONE, NONE, GM, GM};
        double w[] = {0.1, 1, 1, 1, 1, 0.9, 0.2};
        EXPECT(plan(5, 7, f, t, k, w, 0.25, 7, p) == PRUNE_OK);
        EXPECT(p.removed == std::vector<int>({0, 6}) && p.remap == std::vector<int>({-1, 0, 1, 2, 3, 4, -1}));
        // what moves with the edges
        std::vector<int> from(f, f + 7);
        std::vector<double> meas(7 * 7);
        for (int e = 0; e < 7; e++)
            for (int c = 0; c < 7; c++)
                meas[7 * e + c] = 10 * e + c;
        compact(from, 1, p.remap);
        compact(meas, 7, p.remap);
        EXPECT(from == std::vector<int>({0, 1, 2, 3, 4}) && meas.size() == 35 && meas[0] == 10 && meas[34] == 56);
        // strict: w == threshold stays; a NaN weight stays
        w[0] = 0.25, w[6] = nan;
        EXPECT(plan(5, 7, f, t, k, w, 0.25, 7, p) == PRUNE_OK && p.removed.empty());
        // capacity: two to remove, one slot; nothing is decided beyond the count
        w[0] = 0.1, w[6] = 0.2;
        EXPECT(plan(5, 7, f, t, k, w, 0.25, 1, p) == PRUNE_CAPACITY && p.removed.size() == 2);
        EXPECT(plan(5, 7, f, t, k, w, 0.25, 0, p) == PRUNE_CAPACITY && plan(5, 7, f, t, k, w, 0.25, -3, p) == PRUNE_CAPACITY);
        EXPECT(plan(5, 7, f, t, k, w, 0.25, 2, p) == PRUNE_OK);
        // all the closures removed
        EXPECT(plan(5, 7, f, t, k, w, 2.0, 7, p) == PRUNE_OK && p.removed == std::vector<int>({0, 5, 6}));
        EXPECT(plan(5, 7, f, t, k, w, inf, 7, p) == PRUNE_OK && p.removed.size() == 3);
    }
    // the exemption: an edge between consecutive vertices stays whatever its weight, in either direction
    {
        const int f[] = {0, 2, 2, 0}, t[] = {1, 1, 3, 3};
        const int k[] = {GM, GM, GM, GM};
        const double w[] = {0, 0, 0, 0};
        EXPECT(plan(4, 4, f, t, k, w, 0.25, 4, p) == PRUNE_OK && p.removed == std::vector<int>({3}));
    }
    // repeated endpoints: two edges between the same pair, one goes; both go; a self-loop goes
    {
        const int f[] = {0, 1, 2, 2, 2}, t[] = {1, 2, 0, 0, 2};
        const int k[] = {NONE, NONE, GM, GM, GM};
        const double w1[] = {1, 1, 0.1, 0.9, 0.9}, w2[] = {1, 1, 0.1, 0.1, 0.1};
        EXPECT(plan(3, 5, f, t, k, w1, 0.25, 5, p) == PRUNE_OK && p.removed == std::vector<int>({2}));
        EXPECT(p.remap == std::vector<int>({0, 1, -1, 2, 3}));
        EXPECT(plan(3, 5, f, t, k, w2, 0.25, 5, p) == PRUNE_OK && p.removed == std::vector<int>({2, 3, 4}));
    }
    // every edge removed, and the removal that disconnects: vertex 2 hangs on a closure alone (a graph read from a file)
    {
        const int f[] = {0, 0}, t[] = {1, 2};
        const int k[] = {NONE, GM};
        const double w[] = {1, 0.1};
        EXPECT(plan(3, 2, f, t, k, w, 0.25, 2, p) == PRUNE_DISCONNECTS && p.orphan == 2 && p.removed == std::vector<int>({1}));
        EXPECT(plan(3, 2, f, t, k, w, 0.05, 2, p) == PRUNE_OK && p.removed.empty());
        const int f2[] = {0, 3}, t2[] = {2, 1}, k2[] = {GM, GM};
        EXPECT(plan(4, 2, f2, t2, k2, w, 2.0, 2, p) == PRUNE_DISCONNECTS && p.orphan == 1 && p.removed.size() == 2);
        // capacity is reported before reachability
        EXPECT(plan(4, 2, f2, t2, k2, w, 2.0, 1, p) == PRUNE_CAPACITY);
    }
    // a long chain with a closure from every tenth vertex to vertex 0
    {
        const int nv = 5000;
        std::vector<int> f, t, k;
        std::vector<double> w;
        for (int v = 1; v < nv; v++) {
            f.push_back(v - 1), t.push_back(v), k.push_back(NONE), w.push_back(1.0);
            if (v % 10 == 0)
                f.push_back(v), t.push_back(0), k.push_back(GM), w.push_back(v % 20 ? 0.9 : 0.1);
        }
        EXPECT(plan(nv, (int)f.size(), f.data(), t.data(), k.data(), w.data(), 0.25, nv, p) == PRUNE_OK);
        EXPECT(p.removed.size() == 249);
        int kept = 0;
        for (size_t e = 0; e < f.size(); e++)
            EXPECT(p.remap[e] == (w[e] < 0.25 ? -1 : kept++));
    }
    std::puts("pg prune plan check ok");
    return 0;
}
