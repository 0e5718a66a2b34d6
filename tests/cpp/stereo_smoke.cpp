// The reference's dense-stereo sequence through the adaptor (src/StereoCV.cpp:21-59,227-250):
// StereoProcess(l, r) -> stereoMatch(iter) -> reprojectDisparity, once as the reference calls it and once with
// metricDisparity.  Usage: stereo_smoke <left pattern> <right pattern> <iter> <out prefix>; writes
// <prefix>.disp (int16), <prefix>_{ref,metric}.xyz / .bgr (float32 triples).
#include <cstdio>
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
    if (argc != 5)
        return 2;
    StereoProcess sp(argv[1], argv[2]);
    Mat disp = sp.stereoMatch(std::atoi(argv[3]));
    if (disp.empty())
        return 3;
    std::vector<Point3f> pts, cols;
    const size_t n = (size_t)disp.rows * disp.cols;
    if (!dump(argv[4], ".disp", disp.data, n * 2))
        return 4;
    for (int metric = 0; metric < 2; metric++) {
        sp.metricDisparity = metric != 0;
        sp.reprojectDisparity(disp, pts, cols);
        if (!dump(argv[4], metric ? "_metric.xyz" : "_ref.xyz", pts.data(), pts.size() * sizeof(Point3f)) ||
            !dump(argv[4], metric ? "_metric.bgr" : "_ref.bgr", cols.data(), cols.size() * sizeof(Point3f)))
            return 5;
        std::printf("%s: %zu points\n", metric ? "metric" : "reference", pts.size());
    }
    std::printf("stereo smoke ok\n");
    return 0;
}
