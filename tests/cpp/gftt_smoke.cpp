// The GFTT switch of visualSLAM through the adaptors, on a stereo pair read from two image files (PNG / PPM / PGM):
// gfttKeypointExtractor (cv::goodFeaturesToTrack) and stereoTriangulate with DENSE_FLAG && GFTT_FLAG.
// Usage: gftt_smoke <left> <right> fx fy cx cy baseline maxCorners quality minDistance.  Checks, and fails with a message when one
// does not hold:
//   * with GFTT_FLAG off -- and the gftt members set all the same -- stereoTriangulate returns exactly what an object whose GFTT
//     members were never touched returns;
//   * gfttKeypointExtractor: size 3 (the block size), angle -1, positive responses in descending order, no more than maxCorners, no
//     two key points closer than minDistance;
//   * with the flag on every reference point is one of the extractor's key points and every triangulated depth is positive; with
//     FAST_FLAG on as well the FAST source wins.
// Prints "# gftt <n>" with one line "x y response" per key point, "# on <n>" with one line "x y X Y Z" per pair (%.9g: every float
// survives the round trip), and "gftt smoke ok" at the end.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>
#include <vector>

#include "svo_compat/visualSLAM.hpp"

using namespace svo_compat;

#define FAIL(...)                          \
    do {                                   \
        std::fprintf(stderr, __VA_ARGS__); \
        std::fprintf(stderr, "\n");        \
        return 1;                          \
    } while (0)

static bool load(const char *path, Mat &im)
{
    int w = 0, h = 0, c = 0;
    if (svo_io_image_info(path, &w, &h, &c) != SVO_OK)
        return false;
    im = Mat(h, w, CV_8UC3);
    return svo_io_read_image(path, 3, im.data, (size_t)w * h * 3, &w, &h) == SVO_OK;
}

static void configure(visualSLAM &s, char **argv)
{
    s.focal_x = std::atof(argv[3]);
    s.focal_y = std::atof(argv[4]);
    s.cx = std::atof(argv[5]);
    s.cy = std::atof(argv[6]);
    s.baseline = std::atof(argv[7]);
    s.ransacSeed = 5;
}

int main(int argc, char **argv)
{
    if (argc != 11)
        return 2;
    Mat left, right;
    if (!load(argv[1], left) || !load(argv[2], right)) {
        std::fprintf(stderr, "%s\n", svo_last_error());
        return 3;
    }
    const int max_corners = std::atoi(argv[8]);
    const double quality = std::atof(argv[9]), min_distance = std::atof(argv[10]);

    // flag off: the same calls as ever
    visualSLAM plain, off;
    if (plain.GFTT_FLAG || plain.gfttMaxCorners != 1000 || plain.gfttQuality != 0.01 || plain.gfttMinDistance != 10 || !plain.DENSE_FLAG)
        FAIL("the defaults moved");
    configure(plain, argv);
    configure(off, argv);
    off.gfttMaxCorners = max_corners;
    off.gfttQuality = quality;
    off.gfttMinDistance = min_distance;
    std::vector<Point3f> a3, b3;
    std::vector<Point2f> a2, b2;
    plain.stereoTriangulate(left, right, a3, a2);
    off.stereoTriangulate(left, right, b3, b2);
    if (a2.empty() || a2.size() != b2.size() || a3.size() != b3.size())
        FAIL("flag off: %zu and %zu reference points", a2.size(), b2.size());
    for (size_t i = 0; i < a2.size(); i++)
        if (a2[i].x != b2[i].x || a2[i].y != b2[i].y || a3[i].x != b3[i].x || a3[i].y != b3[i].y || a3[i].z != b3[i].z)
            FAIL("flag off: pair %zu differs from the untouched object's", i);

    // the extractor by itself
    visualSLAM on;
    configure(on, argv);
    on.GFTT_FLAG = true;
    on.gfttMaxCorners = max_corners;
    on.gfttQuality = quality;
    on.gfttMinDistance = min_distance;
    std::vector<KeyPoint> kps = on.gfttKeypointExtractor(left);
    if (kps.size() < 8 || (max_corners > 0 && kps.size() > (size_t)max_corners))
        FAIL("%zu GFTT key points", kps.size());
    std::set<std::pair<float, float>> corners;
    for (size_t i = 0; i < kps.size(); i++) {
        const KeyPoint &k = kps[i];
        if (k.size != 3.f || k.angle != -1.f || !(k.response > 0.f))
            FAIL("key point %zu: size %g angle %g response %g", i, k.size, k.angle, k.response);
        if (i && k.response > kps[i - 1].response)
            FAIL("key point %zu is out of response order", i);
        for (size_t j = 0; j < i; j++) {
            const double dx = k.pt.x - kps[j].pt.x, dy = k.pt.y - kps[j].pt.y;
            if (dx * dx + dy * dy < min_distance * min_distance)
                FAIL("key points %zu and %zu are closer than %g", j, i, min_distance);
        }
        corners.insert({k.pt.x, k.pt.y});
    }
    std::printf("# gftt %zu\n", kps.size());
    for (const KeyPoint &p : kps)
        std::printf("%.9g %.9g %.9g\n", p.pt.x, p.pt.y, p.response);

    // flag on: reference points from the extractor, then the same LK -> FmatThresholding -> triangulation
    std::vector<Point3f> p3;
    std::vector<Point2f> p2;
    on.stereoTriangulate(left, right, p3, p2);
    if (p2.size() < 8 || p3.size() != p2.size() || on.colors.size() != p2.size())
        FAIL("flag on: %zu reference points, %zu 3-D points", p2.size(), p3.size());
    std::printf("# on %zu\n", p2.size());
    for (size_t i = 0; i < p2.size(); i++) {
        std::printf("%.9g %.9g %.9g %.9g %.9g\n", p2[i].x, p2[i].y, p3[i].x, p3[i].y, p3[i].z);
        if (!corners.count({p2[i].x, p2[i].y}))
            FAIL("flag on: reference point %zu (%g, %g) is no GFTT key point", i, p2[i].x, p2[i].y);
        if (!(p3[i].z > 0.f))
            FAIL("flag on: point %zu has depth %g", i, p3[i].z);
    }

    // both flags: FAST is asked first
    visualSLAM fast, both;
    configure(fast, argv);
    configure(both, argv);
    fast.FAST_FLAG = both.FAST_FLAG = both.GFTT_FLAG = true;
    fast.fastThreshold = both.fastThreshold = 20;
    std::vector<Point3f> f3, g3;
    std::vector<Point2f> f2, g2;
    fast.stereoTriangulate(left, right, f3, f2);
    both.stereoTriangulate(left, right, g3, g2);
    if (f2.size() != g2.size())
        FAIL("both flags: %zu reference points, FAST alone %zu", g2.size(), f2.size());
    for (size_t i = 0; i < f2.size(); i++)
        if (f2[i].x != g2[i].x || f2[i].y != g2[i].y)
            FAIL("both flags: pair %zu is not FAST's", i);
    std::printf("gftt smoke ok\n");
    return 0;
}
