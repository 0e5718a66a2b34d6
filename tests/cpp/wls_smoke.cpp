// The reference's dense-stereo call with the filter its author wrote around the matcher (src/StereoCV.cpp:25-28,51-59,
// commented out upstream) through the adaptor: StereoProcess(l, r) -> stereoMatch(iter) with WLS_FLAG clear (the code it
// runs today) and set (right matcher, left-right confidence, fast global smoother; lambda 400, sigma 0.4 as upstream sets them).
// Usage: wls_smoke <left pattern> <right pattern> <iter> <out prefix>; writes <prefix>.raw and <prefix>.wls (int16) and
// <prefix>.conf (float32).
#include <cstdio>
#include <cstdlib>

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
    if (sp.WLS_FLAG || sp.lambda != 400 || sp.sigma != 0.4)
        return 6;
    Mat raw = sp.stereoMatch(std::atoi(argv[3]));
    if (raw.empty() || !sp.confidenceMap.empty())
        return 3;
    sp.WLS_FLAG = true;
    Mat filt = sp.stereoMatch(std::atoi(argv[3]));
    if (filt.empty() || sp.confidenceMap.empty() || sp.confidenceMap.rows != filt.rows || sp.confidenceMap.cols != filt.cols)
        return 4;
    const size_t n = (size_t)filt.rows * filt.cols;
    if (!dump(argv[4], ".raw", raw.data, n * 2) || !dump(argv[4], ".wls", filt.data, n * 2) ||
        !dump(argv[4], ".conf", sp.confidenceMap.data, n * 4))
        return 5;
    std::printf("wls smoke ok: %d x %d\n", filt.cols, filt.rows);
    return 0;
}
