// visualSLAM::stereoTriangulate with DENSE_FLAG = false (the ORB branch) and the pairing chosen by CROSS_CHECK_FLAG /
// EPIPOLAR_GATE_FLAG, through the adaptor on a stereo pair read from two image files (PNG / PPM / PGM).
// Usage: match_ext_smoke <left> <right> <plain|cross|gate|both> [epipolarRows maxDisparity].  Prints one line per pair:
//   x y X Y Z    (2-D point in the left image, 3-D point; %.9g: every float survives the round trip)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "svo_compat/visualSLAM.hpp"

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
    if (argc != 4 && argc != 6)
        return 2;
    Mat left, right;
    if (!load(argv[1], left) || !load(argv[2], right)) {
        std::fprintf(stderr, "%s\n", svo_last_error());
        return 3;
    }
    visualSLAM slam;
    slam.DENSE_FLAG = false;
    slam.CROSS_CHECK_FLAG = !std::strcmp(argv[3], "cross") || !std::strcmp(argv[3], "both");
    slam.EPIPOLAR_GATE_FLAG = !std::strcmp(argv[3], "gate") || !std::strcmp(argv[3], "both");
    if (!slam.CROSS_CHECK_FLAG && !slam.EPIPOLAR_GATE_FLAG && std::strcmp(argv[3], "plain"))
        return 2;
    if (argc == 6) {
        slam.epipolarRows = (float)std::atof(argv[4]);
        slam.maxDisparity = (float)std::atof(argv[5]);
    }
    std::vector<Point3f> p3;
    std::vector<Point2f> p2;
    slam.stereoTriangulate(left, right, p3, p2);
    if (p3.size() != p2.size())
        return 4;
    std::printf("# stereoTriangulate, pairing %s: %zu pairs of at most %d features\n", argv[3], p2.size(), slam.orbFeatures);
    for (size_t i = 0; i < p2.size(); i++)
        std::printf("%.9g %.9g %.9g %.9g %.9g\n", p2[i].x, p2[i].y, p3[i].x, p3[i].y, p3[i].z);
    return 0;
}
