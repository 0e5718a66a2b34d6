// The Star detector and the Star + BRIEF branch of visualSLAM::stereoTriangulate (src/triangulation.cpp:79-80, the commented pair)
// through the adaptor, on a stereo pair read from two image files (PNG / PPM / PGM).
// Usage: star_brief_smoke <left> <right> fx fy cx cy baseline starMaxSize starResponseThreshold.  Prints
//   "# star <n>" and one line "x y size response" per key point of starKeypointExtractor(left),
//   "# pairs <n>" and one line "x y X Y Z" per pair: ref2dPts and ref3dPts of stereoTriangulate with DENSE_FLAG = false,
//   STAR_FLAG = true,
//   "star brief smoke ok"
// (%.9g: every float survives the round trip).
#include <cstdio>
#include <cstdlib>
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
    if (argc != 10)
        return 2;
    Mat left, right;
    if (!load(argv[1], left) || !load(argv[2], right)) {
        std::fprintf(stderr, "%s\n", svo_last_error());
        return 3;
    }
    visualSLAM slam;
    if (slam.STAR_FLAG || !slam.DENSE_FLAG || slam.SURF_FLAG || slam.starMaxSize != 45 || slam.starResponseThreshold != 30)
        return 6;
    slam.focal_x = std::atof(argv[3]);
    slam.focal_y = std::atof(argv[4]);
    slam.cx = std::atof(argv[5]);
    slam.cy = std::atof(argv[6]);
    slam.baseline = std::atof(argv[7]);
    slam.starMaxSize = std::atoi(argv[8]);
    slam.starResponseThreshold = std::atoi(argv[9]);
    if (!slam.starKeypointExtractor(Mat()).empty())
        return 7;
    const std::vector<KeyPoint> kps = slam.starKeypointExtractor(left);
    std::printf("# star %zu\n", kps.size());
    for (const KeyPoint &k : kps) {
        if (k.angle != -1.f || k.octave != 0)
            return 5;
        std::printf("%.9g %.9g %.9g %.9g\n", k.pt.x, k.pt.y, k.size, k.response);
    }
    slam.DENSE_FLAG = false;
    slam.STAR_FLAG = true;
    std::vector<Point3f> p3;
    std::vector<Point2f> p2;
    slam.stereoTriangulate(left, right, p3, p2);
    if (p3.size() != p2.size() || slam.colors.size() != p2.size())
        return 4;
    std::printf("# pairs %zu\n", p2.size());
    for (size_t i = 0; i < p2.size(); i++)
        std::printf("%.9g %.9g %.9g %.9g %.9g\n", p2[i].x, p2[i].y, p3[i].x, p3[i].y, p3[i].z);
    std::puts("star brief smoke ok");
    return 0;
}
