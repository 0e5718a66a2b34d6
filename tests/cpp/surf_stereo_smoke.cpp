// The two SURF users of the reference through the adaptors, on a stereo pair read from two image files (PNG / PPM / PGM):
// visualOdometry::stereoTriangulate and ::relocalizeFrames (src/bundleAdjust.cpp:236-317, 384-404) and the SURF branch of
// visualSLAM::stereoTriangulate (include/trangulation.h:32-61).
// Usage: surf_stereo_smoke <left> <right> fx fy cx cy baseline [surfHessian of visualOdometry [surfHessian of visualSLAM]].  Prints
//   "NULL IMG", upstream's line for the null image that stereoTriangulate is given first,
//   "# vo <n>" and one line "x y X Y Z" per pair: ref2dPts and ref3dPts of visualOdometry::stereoTriangulate,
//   "# transform" with the twelve doubles of the 3x4 inv_transform (%.17g), "# reloc <n>" and one line "x y X Y Z" per pair:
//   ftrPts and pts3d of relocalizeFrames,
//   "# slam <n>" and one line "x y X Y Z" per pair of visualSLAM::stereoTriangulate with DENSE_FLAG = false, SURF_FLAG = true,
//   "# surfFeatures <n>": the key points surfFeatures finds in the left image
// (%.9g: every float survives the round trip).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "svo_compat/bundleAdjust.hpp"
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

static void print_pairs(const char *name, const std::vector<Point2f> &p2, const std::vector<Point3f> &p3)
{
    std::printf("# %s %zu\n", name, p2.size());
    for (size_t i = 0; i < p2.size(); i++)
        std::printf("%.9g %.9g %.9g %.9g %.9g\n", p2[i].x, p2[i].y, p3[i].x, p3[i].y, p3[i].z);
}

int main(int argc, char **argv)
{
    if (argc < 8 || argc > 10)
        return 2;
    Mat left, right;
    if (!load(argv[1], left) || !load(argv[2], right)) {
        std::fprintf(stderr, "%s\n", svo_last_error());
        return 3;
    }
    const double fx = std::atof(argv[3]), fy = std::atof(argv[4]), cx = std::atof(argv[5]), cy = std::atof(argv[6]);
    visualOdometry vo;
    if (vo.surfHessian != 500 || vo.baseline != 0.54)
        return 6;
    vo.baseline = std::atof(argv[7]);
    vo.K = Mat::zeros(3, 3, CV_64F);
    vo.K.at<double>(0, 0) = fx;
    vo.K.at<double>(1, 1) = fy;
    vo.K.at<double>(0, 2) = cx;
    vo.K.at<double>(1, 2) = cy;
    vo.K.at<double>(2, 2) = 1;
    if (argc >= 9)
        vo.surfHessian = std::atoi(argv[8]);
    // a null image returns as upstream does, after its "NULL IMG" line: the outputs stay as they are.  First, so that the line
    // stands before every section
    std::vector<Point3f> q3(1);
    std::vector<Point2f> q2(1);
    vo.stereoTriangulate(Mat(), right, q3, q2);
    if (q3.size() != 1 || q2.size() != 1)
        return 7;
    std::vector<Point3f> p3;
    std::vector<Point2f> p2;
    vo.stereoTriangulate(left, right, p3, p2);
    if (p3.size() != p2.size())
        return 4;
    print_pairs("vo", p2, p3);
    // relocalizeFrames: a small rotation about y and a translation
    Mat T = Mat::zeros(3, 4, CV_64F);
    const double a = 0.1, t[3] = {0.25, -0.125, 1.5};
    const double R[9] = {std::cos(a), 0, std::sin(a), 0, 1, 0, -std::sin(a), 0, std::cos(a)};
    std::printf("# transform");
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 4; j++) {
            T.at<double>(i, j) = j < 3 ? R[3 * i + j] : t[i];
            std::printf(" %.17g", T.at<double>(i, j));
        }
    std::printf("\n");
    std::vector<Point3f> r3(3);
    std::vector<Point2f> r2(5);
    vo.relocalizeFrames(0, left, right, T, r2, r3);
    if (r3.size() != r2.size())
        return 4;
    print_pairs("reloc", r2, r3);
    // the SURF branch of visualSLAM::stereoTriangulate
    visualSLAM slam;
    if (slam.SURF_FLAG || !slam.DENSE_FLAG || slam.surfHessian != 1200)
        return 6;
    slam.DENSE_FLAG = false;
    slam.SURF_FLAG = true;
    slam.focal_x = fx;
    slam.focal_y = fy;
    slam.cx = cx;
    slam.cy = cy;
    slam.baseline = vo.baseline;
    if (argc >= 10)
        slam.surfHessian = std::atoi(argv[9]);
    std::vector<Point3f> s3;
    std::vector<Point2f> s2;
    slam.stereoTriangulate(left, right, s3, s2);
    if (s3.size() != s2.size() || slam.colors.size() != s2.size())
        return 4;
    print_pairs("slam", s2, s3);
    std::vector<KeyPoint> kps;
    std::vector<float> desc;
    vo.surfFeatures(left, kps, desc);
    if (desc.size() != 64 * kps.size())
        return 5;
    std::printf("# surfFeatures %zu\n", kps.size());
    return 0;
}
