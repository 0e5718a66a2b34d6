// StereoProcess::pclPublish (src/StereoCV.cpp:275-296) through the adaptor on a cloud read from a file.
// Usage: stereo_publish_smoke <in> <out prefix>; <in>: n x 6 float32 (x, y, z, b, g, r as reprojectDisparity leaves
// them); writes <prefix>.xyz and <prefix>.rgb (publishedCloud / publishedColors, float32 triples) and checks that
// pts3d and colorMap came back unchanged.
#include <cstdio>
#include <cstring>
#include <vector>

#include "svo_compat/stereoCV.hpp"

using namespace svo_compat;

static bool dump(const char *prefix, const char *suffix, const void *p, size_t bytes)
{
    char path[1024];
    std::snprintf(path, sizeof(path), "%s%s", prefix, suffix);
    FILE *f = std::fopen(path, "wb");
    if (!f)
        return false;
    const bool ok = std::fwrite(p, 1, bytes, f) == bytes;
    std::fclose(f);
    return ok;
}

int main(int argc, char **argv)
{
    if (argc != 3)
        return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f)
        return 3;
    std::vector<float> raw;
    float buf[6];
    while (std::fread(buf, sizeof(float), 6, f) == 6)
        raw.insert(raw.end(), buf, buf + 6);
    std::fclose(f);
    std::vector<Point3f> pts, cols;
    for (size_t i = 0; i + 6 <= raw.size(); i += 6) {
        pts.emplace_back(raw[i], raw[i + 1], raw[i + 2]);
        cols.emplace_back(raw[i + 3], raw[i + 4], raw[i + 5]);
    }
    const std::vector<Point3f> pts0 = pts, cols0 = cols;
    StereoProcess sp;
    sp.pclPublish(pts, cols);
    for (size_t i = 0; i < pts.size(); i++)
        if (std::memcmp(&pts[i], &pts0[i], sizeof(Point3f)) || std::memcmp(&cols[i], &cols0[i], sizeof(Point3f)))
            return 4;
    if (pts.size() != pts0.size() || sp.publishedCloud.size() != sp.publishedColors.size())
        return 5;
    if (!dump(argv[2], ".xyz", sp.publishedCloud.data(), sp.publishedCloud.size() * sizeof(Point3f)) ||
        !dump(argv[2], ".rgb", sp.publishedColors.data(), sp.publishedColors.size() * sizeof(Point3f)))
        return 6;
    std::printf("publish smoke ok: %zu of %zu points published\n", sp.publishedCloud.size(), pts.size());
    return 0;
}
