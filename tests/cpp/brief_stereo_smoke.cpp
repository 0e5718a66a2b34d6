// StereoProcess::stereoTriangulate (src/StereoCV.cpp:64-121) with BRIEF_FLAG = true -- the reference's own SIFT -> BRIEF ->
// knnMatch -> ratio -> F -> triangulatePoints sequence -- through the adaptor on a stereo pair read from two image files
// (PNG / PPM / PGM).
// Usage: brief_stereo_smoke <left> <right> [fx fy cx cy baseline [siftFeatures [briefBytes]]].  Prints
//   "# pairs <n>" and one line "x1 y1 x2 y2" per pair that passed the ratio test,
//   "# inliers <m>" and one line "x1 y1 x2 y2 X Y Z B G R" per F-inlier (its 3-D point and the colour of the left pixel),
//   "# briefFeatures <k> of <n>": the key points of the left image brief->compute keeps of those SIFT found
// (%.9g: every float survives the round trip).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "svo_compat/stereoCV.hpp"

using namespace svo_compat;

static bool load(const char *path, Mat &im)
{
    int w = 0, h = 0, c = 0;
    if (svo_io_image_info(path, &w, &h, &c) != SVO_OK)
        return false;
    im = Mat(h, w, CV_8UC3);
    return svo_io_read_image(path, 3, im.data, (size_t)w * h * 3, &w, &h) == SVO_OK;
}

int main(int argc, char **argv)
{
    if (argc != 3 && argc != 8 && argc != 9 && argc != 10)
        return 2;
    Mat left, right;
    if (!load(argv[1], left) || !load(argv[2], right)) {
        std::fprintf(stderr, "%s\n", svo_last_error());
        return 3;
    }
    StereoProcess sp;
    sp.BRIEF_FLAG = true;
    if (argc >= 8) {
        sp.focal_x = std::atof(argv[3]);
        sp.focal_y = std::atof(argv[4]);
        sp.cx = std::atof(argv[5]);
        sp.cy = std::atof(argv[6]);
        sp.baseline = std::atof(argv[7]);
    }
    if (argc >= 9)
        sp.siftFeaturesStereo = std::atoi(argv[8]);
    if (argc >= 10)
        sp.briefBytes = std::atoi(argv[9]);
    std::vector<Point3f> out3d;
    sp.stereoTriangulate(left, right, out3d);
    const size_t m = out3d.size();
    if (sp.stereoPairs1.size() != sp.stereoPairs2.size() || sp.stereoInliers1.size() != m || sp.stereoInliers2.size() != m ||
        sp.tri3dPoints.size() != m || sp.color3dMap.size() != m)
        return 4;
    std::printf("# pairs %zu\n", sp.stereoPairs1.size());
    for (size_t i = 0; i < sp.stereoPairs1.size(); i++)
        std::printf("%.9g %.9g %.9g %.9g\n", sp.stereoPairs1[i].x, sp.stereoPairs1[i].y, sp.stereoPairs2[i].x, sp.stereoPairs2[i].y);
    std::printf("# inliers %zu\n", m);
    for (size_t i = 0; i < m; i++)
        std::printf("%.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g\n", sp.stereoInliers1[i].x, sp.stereoInliers1[i].y,
                    sp.stereoInliers2[i].x, sp.stereoInliers2[i].y, out3d[i].x, out3d[i].y, out3d[i].z, sp.color3dMap[i].x,
                    sp.color3dMap[i].y, sp.color3dMap[i].z);
    // brief->compute on one image: the filtered key points leave the vector
    std::vector<KeyPoint> kps;
    std::vector<float> unused;
    sp.siftFeatures(left, kps, unused, sp.siftFeaturesStereo);
    const size_t found = kps.size();
    std::vector<uint8_t> desc;
    sp.briefFeatures(left, kps, desc);
    if (desc.size() != kps.size() * (size_t)sp.briefBytes || kps.size() > found)
        return 5;
    std::printf("# briefFeatures %zu of %zu\n", kps.size(), found);
    return 0;
}
