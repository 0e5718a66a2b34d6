// visualSLAM::stereoTriangulate with DENSE_FLAG = false (src/triangulation.cpp:104-166: ORB + BFMatcher + ratio test, then
// colours and triangulation) through the adaptor on a stereo pair read from two image files (PNG / PPM / PGM).
// Usage: sparse_triangulate_smoke <left> <right> [orbFeatures].  Prints one line per surviving pair:
//   x y X Y Z B G R    (2-D point in the left image, 3-D point, colour; %.9g: every float survives the round trip)
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
    if (argc != 3 && argc != 4)
        return 2;
    Mat left, right;
    if (!load(argv[1], left) || !load(argv[2], right)) {
        std::fprintf(stderr, "%s\n", svo_last_error());
        return 3;
    }
    visualSLAM slam;
    slam.DENSE_FLAG = false;
    if (argc == 4)
        slam.orbFeatures = std::atoi(argv[3]);
    std::vector<Point3f> p3;
    std::vector<Point2f> p2;
    slam.stereoTriangulate(left, right, p3, p2);
    if (p3.size() != p2.size() || slam.colors.size() != p2.size())
        return 4;
    std::printf("# sparse stereoTriangulate: %zu pairs of at most %d features\n", p2.size(), slam.orbFeatures);
    for (size_t i = 0; i < p2.size(); i++)
        std::printf("%.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g\n", p2[i].x, p2[i].y, p3[i].x, p3[i].y, p3[i].z, slam.colors[i].x,
                    slam.colors[i].y, slam.colors[i].z);
    return 0;
}
