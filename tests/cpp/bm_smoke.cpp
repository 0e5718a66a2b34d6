// The dense-stereo call through the adaptor with the block matcher in StereoSGBM's place: StereoProcess(l, r) ->
// stereoMatch(iter) with BM_FLAG set (svo_bm_compute), then with WLS_FLAG set as well (svo_bm_wls_compute; lambda 400, sigma 0.4
// as upstream sets them).  Usage: bm_smoke <left pattern> <right pattern> <iter> <out prefix>; writes <prefix>.bm and
// <prefix>.wls (int16) and <prefix>.conf (float32).
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
    const svo_bm_params &b = sp.bmParams;
    if (sp.BM_FLAG || sp.WLS_FLAG || b.min_disparity != 1 || b.num_disparities != 96 || b.speckle_window_size != 3000 ||
        b.speckle_range != 5 || b.block_size != 21 || b.pre_filter_type != SVO_BM_PREFILTER_XSOBEL || b.pre_filter_size != 9 ||
        b.pre_filter_cap != 31 || b.texture_threshold != 10 || b.uniqueness_ratio != 15 || b.disp12_max_diff != -1)
        return 6;
    sp.BM_FLAG = true;
    Mat raw = sp.stereoMatch(std::atoi(argv[3]));
    if (raw.empty() || !sp.confidenceMap.empty())
        return 3;
    sp.WLS_FLAG = true;
    Mat filt = sp.stereoMatch(std::atoi(argv[3]));
    if (filt.empty() || sp.confidenceMap.empty() || sp.confidenceMap.rows != filt.rows || sp.confidenceMap.cols != filt.cols)
        return 4;
    const size_t n = (size_t)filt.rows * filt.cols;
    if (!dump(argv[4], ".bm", raw.data, n * 2) || !dump(argv[4], ".wls", filt.data, n * 2) ||
        !dump(argv[4], ".conf", sp.confidenceMap.data, n * 4))
        return 5;
    std::printf("bm smoke ok: %d x %d\n", filt.cols, filt.rows);
    return 0;
}
