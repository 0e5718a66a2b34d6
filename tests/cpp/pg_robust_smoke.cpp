// globalPoseGraph::setLoopClosureKernel and pruneLoopClosures through the adaptor: a lap of 24 poses on a circle with exact
// odometry, one false closure (vertex 12 -> 3, identity measurement) and the true one (the last pose coincides with pose 0).  With
// the Geman-McClure kernel on the closures the optimisation down-weights the false edge, the prune removes exactly that edge, and
// the second optimisation brings the lap back.  Usage: pg_robust_smoke <out>; writes the removed index and the edge counts.
#include <cmath>
#include <cstdio>
#include <vector>

#include "svo_compat/poseGraph.hpp"

using namespace svo_compat;

static Isometry3d pose_on_circle(int k, int n)
{
    const double kPi = 3.14159265358979323846;
    const double a = 2.0 * kPi * k / n, c = std::cos(a), s = std::sin(a), radius = 0.5;
    Isometry3d T = Isometry3d::Identity();
    T(0, 0) = c, T(0, 2) = s, T(2, 0) = -s, T(2, 2) = c;  // rotation about y
    T(0, 3) = radius * s, T(2, 3) = radius * (1.0 - c);
    return T;
}

int main(int argc, char **argv)
{
    if (argc != 2)
        return 2;
    const int n = 24;
    globalPoseGraph pg;
    pg.initializeGraph();
    pg.writeResultFile = false;
    int wrong = -1;
    for (int k = 1; k <= n; k++) {
        const Isometry3d T = k == n ? Isometry3d::Identity() : pose_on_circle(k, n);
        pg.augmentNode(T, T);
        if (k == 7)
            pg.setLoopClosureKernel(SVO_PG_ROBUST_GEMAN_MCCLURE, 1e-3);
        if (k == 12) {
            wrong = pg.numEdges();
            pg.addLoopClosure(T, 3);
        }
    }
    pg.addLoopClosure(Isometry3d::Identity(), 0);
    const int before = pg.numEdges();
    int kind = -1;
    double delta = -1;
    check(svo_pg_get_robust_kernel(pg.handle(), wrong, &kind, &delta));
    if (kind != SVO_PG_ROBUST_GEMAN_MCCLURE || delta != 1e-3)
        return 3;
    check(svo_pg_get_robust_kernel(pg.handle(), 0, &kind, &delta));  // an odometry edge
    if (kind != SVO_PG_ROBUST_NONE)
        return 4;
    pg.globalOptimize();
    const std::vector<int> removed = pg.pruneLoopClosures(0.25);
    if (removed.size() != 1 || removed[0] != wrong || pg.numEdges() != before - 1)
        return 5;
    const std::vector<Isometry3d> X = pg.globalOptimize();
    if ((int)X.size() != n + 1)
        return 6;
    if (!pg.pruneLoopClosures(0.25).empty())
        return 7;
    FILE *f = std::fopen(argv[1], "w");
    if (!f)
        return 8;
    std::fprintf(f, "%d %d %d\n", removed[0], before, pg.numEdges());
    std::fclose(f);
    std::printf("pg robust smoke ok: removed edge %d of %d\n", removed[0], before);
    return 0;
}
