// visualSLAM::getLCMeasurement (dump.cpp:331-348) and globalPoseGraph::addLoopClosure with MEASURED_LC_FLAG / INFORMATION_FLAG
// through the adaptors.  Usage: closure_measure_smoke <newest> <matched> <w> <h> <points> <n> <fx> <fy> <cx> <cy> <out>
// newest / matched: h x w x 1 uint8 images; points: n records of 5 float32 (x y X Y Z: the newest frame's points and their
// positions in its camera frame).  Writes <out>: the 7 doubles of the measurement as the pose graph stores it (get_edge of the
// closure it adds), then the 21 doubles of that edge's information, then tracked and inlier counts as doubles.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "svo_compat/visualSLAM.hpp"

using namespace svo_compat;

static bool read_all(const char *path, void *p, size_t bytes)
{
    FILE *f = std::fopen(path, "rb");
    if (!f)
        return false;
    const bool ok = std::fread(p, 1, bytes, f) == bytes;
    std::fclose(f);
    return ok;
}

int main(int argc, char **argv)
{
    if (argc != 12)
        return 2;
    const int w = std::atoi(argv[3]), h = std::atoi(argv[4]), n = std::atoi(argv[6]);
    Mat a(h, w, CV_8UC1), b(h, w, CV_8UC1);
    std::vector<float> rec((size_t)n * 5);
    if (!read_all(argv[1], a.data, (size_t)w * h) || !read_all(argv[2], b.data, (size_t)w * h) ||
        !read_all(argv[5], rec.data(), rec.size() * sizeof(float)))
        return 3;
    visualSLAM slam;
    slam.focal_x = std::atof(argv[7]);
    slam.focal_y = std::atof(argv[8]);
    slam.cx = std::atof(argv[9]);
    slam.cy = std::atof(argv[10]);
    slam.ransacSeed = 11;
    std::vector<Point2f> pts;
    std::vector<Point3f> xyz;
    for (int i = 0; i < n; i++) {
        pts.emplace_back(rec[5 * i], rec[5 * i + 1]);
        xyz.emplace_back(rec[5 * i + 2], rec[5 * i + 3], rec[5 * i + 4]);
    }
    if (!slam.getLCMeasurement(a, b, pts, xyz))
        return 4;
    // a three-vertex graph whose closure carries the measurement and a weight
    globalPoseGraph &pg = slam.poseGraph;
    pg.initializeGraph();
    Isometry3d T = Isometry3d::Identity();
    T(2, 3) = 1.0;
    pg.augmentNode(T, T);
    T(2, 3) = 2.0;
    pg.augmentNode(T, T);
    pg.addLoopClosure(slam.lcMeasurementT, 0);  // the reference's behaviour: T is not read
    pg.MEASURED_LC_FLAG = true;
    pg.INFORMATION_FLAG = true;
    for (int k = 0; k < 6; k++)
        pg.information(k, k) = k < 3 ? 50.0 : 200.0;
    pg.information(0, 4) = pg.information(4, 0) = 3.0;
    pg.addLoopClosure(slam.lcMeasurementT, 0);
    if (pg.numEdges() != 4)
        return 5;
    double out[7 + 7 + 21 + 2];
    int from = -1, to = -1;
    check(svo_pg_get_edge(pg.handle(), 2, &from, &to, out));
    check(svo_pg_get_edge(pg.handle(), 3, &from, &to, out + 7));
    check(svo_pg_get_edge_information(pg.handle(), 3, out + 14));
    if (from != 2 || to != 0)
        return 6;
    out[35] = slam.lcMeasurementTracked;
    out[36] = slam.lcMeasurementInliers;
    pg.optimizeIterations = 3;
    pg.writeResultFile = false;
    if (pg.globalOptimize().size() != 3)
        return 7;
    FILE *f = std::fopen(argv[11], "wb");
    if (!f || std::fwrite(out, sizeof(double), 37, f) != 37)
        return 8;
    std::fclose(f);
    std::printf("closure measure smoke ok: %d tracked, %d inliers\n", slam.lcMeasurementTracked, slam.lcMeasurementInliers);
    return 0;
}
