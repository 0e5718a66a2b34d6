// StereoProcess::voxelDownSample and pclPublish with voxelLeaf through the adaptor on a cloud read from a file.
// Usage: voxel_smoke <in> <out prefix> <leaf> <publish leaf>; <in>: n x 6 float32 (x, y, z, b, g, r as reprojectDisparity leaves
// them).  Writes <prefix>.xyz / <prefix>.bgr (the down-sampled cloud, float32 triples) and <prefix>.pub.xyz / <prefix>.pub.rgb
// (publishedCloud / publishedColors of pclPublish with voxelLeaf = <publish leaf> on the ORIGINAL cloud), and checks that
// voxelLeaf = 0 publishes what it published before the field existed: the same as a second adaptor that never touched it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "svo_compat/stereoCV.hpp"

using namespace svo_compat;

static bool dump(const char *prefix, const char *suffix, const std::vector<Point3f> &v)
{
    char path[1024];
    std::snprintf(path, sizeof(path), "%s%s", prefix, suffix);
    FILE *f = std::fopen(path, "wb");
    if (!f)
        return false;
    const bool ok = std::fwrite(v.data(), sizeof(Point3f), v.size(), f) == v.size();
    std::fclose(f);
    return ok;
}

static bool same(const std::vector<Point3f> &a, const std::vector<Point3f> &b)
{
    return a.size() == b.size() && (a.empty() || !std::memcmp(a.data(), b.data(), a.size() * sizeof(Point3f)));
}

int main(int argc, char **argv)
{
    if (argc != 5)
        return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f)
        return 3;
    std::vector<Point3f> pts0, cols0;
    float buf[6];
    while (std::fread(buf, sizeof(float), 6, f) == 6) {
        pts0.emplace_back(buf[0], buf[1], buf[2]);
        cols0.emplace_back(buf[3], buf[4], buf[5]);
    }
    std::fclose(f);
    const double leaf = std::atof(argv[3]), publish_leaf = std::atof(argv[4]);

    StereoProcess sp;
    if (sp.voxelLeaf != 0)
        return 4;
    std::vector<Point3f> pts = pts0, cols = cols0;
    sp.voxelDownSample(pts, cols, leaf);
    if (pts.size() != cols.size() || pts.size() > pts0.size())
        return 5;
    if (!dump(argv[2], ".xyz", pts) || !dump(argv[2], ".bgr", cols))
        return 6;
    const size_t rows = pts.size();

    pts = pts0, cols = cols0;
    sp.pclPublish(pts, cols);  // voxelLeaf == 0
    const std::vector<Point3f> plain = sp.publishedCloud, plain_rgb = sp.publishedColors;
    sp.voxelLeaf = publish_leaf;
    sp.pclPublish(pts, cols);
    if (!same(pts, pts0) || !same(cols, cols0))
        return 7;
    if (!dump(argv[2], ".pub.xyz", sp.publishedCloud) || !dump(argv[2], ".pub.rgb", sp.publishedColors))
        return 8;
    const size_t thinned = sp.publishedCloud.size();
    sp.voxelLeaf = 0;
    sp.pclPublish(pts, cols);
    if (!same(sp.publishedCloud, plain) || !same(sp.publishedColors, plain_rgb))
        return 9;
    if (!dump(argv[2], ".plain.xyz", plain) || !dump(argv[2], ".plain.rgb", plain_rgb))
        return 10;
    std::printf("voxel smoke ok: %zu of %zu points after the down-sample, %zu published with the leaf, %zu without\n", rows, pts0.size(), thinned, plain.size());
    return 0;
}
