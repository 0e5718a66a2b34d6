// The FAST switch of visualSLAM through the adaptors, on a stereo pair read from two image files (PNG / PPM / PGM):
// fastKeypointExtractor (src/ANMS.cpp:69-82) and stereoTriangulate with DENSE_FLAG && FAST_FLAG.
// Usage: fast_anms_smoke <left> <right> fx fy cx cy baseline fastThreshold fastKeep.  Checks, and fails with a message when one does
// not hold:
//   * with FAST_FLAG off -- and fastThreshold / fastKeep set all the same -- stereoTriangulate returns exactly what an object whose
//     FAST members were never touched returns;
//   * with the flag on, for fastKeep = 0 and for the fastKeep given: every reference point is one of fastKeypointExtractor's key
//     points of the left image, and every triangulated depth is positive;
//   * fastKeypointExtractor: size 7, angle -1, row-major order and response >= 1 without ANMS; with it no more key points than
//     without, in descending response order, each of them one of the plain detector's.
// Prints "# fast <n>", "# anms <n>" with one line "x y response" per key point, "# on0 <n>" and "# on1 <n>" with one line "x y X Y Z"
// per pair of the two runs with the flag on (%.9g: every float survives the round trip), and "fast anms smoke ok" at the end.
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

static void print_kps(const char *name, const std::vector<KeyPoint> &k)
{
    std::printf("# %s %zu\n", name, k.size());
    for (const KeyPoint &p : k)
        std::printf("%.9g %.9g %.9g\n", p.pt.x, p.pt.y, p.response);
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
    const int thr = std::atoi(argv[8]), keep = std::atoi(argv[9]);

    // flag off: the same calls as ever
    visualSLAM plain, off;
    if (plain.FAST_FLAG || plain.fastThreshold != 1 || plain.fastKeep != 0 || !plain.DENSE_FLAG)
        FAIL("the defaults moved");
    configure(plain, argv);
    configure(off, argv);
    off.fastThreshold = thr;
    off.fastKeep = keep;
    std::vector<Point3f> a3, b3;
    std::vector<Point2f> a2, b2;
    plain.stereoTriangulate(left, right, a3, a2);
    off.stereoTriangulate(left, right, b3, b2);
    if (a2.empty() || a2.size() != b2.size() || a3.size() != b3.size() || plain.colors.size() != off.colors.size())
        FAIL("flag off: %zu and %zu reference points", a2.size(), b2.size());
    for (size_t i = 0; i < a2.size(); i++)
        if (a2[i].x != b2[i].x || a2[i].y != b2[i].y || a3[i].x != b3[i].x || a3[i].y != b3[i].y || a3[i].z != b3[i].z ||
            plain.colors[i].x != off.colors[i].x || plain.colors[i].y != off.colors[i].y || plain.colors[i].z != off.colors[i].z)
            FAIL("flag off: pair %zu differs from the untouched object's", i);
    // the grid's points, not corners: the switch was not taken
    std::vector<KeyPoint> grid = plain.denseKeypointExtractor(left, plain.gridStep);
    std::set<std::pair<float, float>> on_grid;
    for (const KeyPoint &k : grid)
        on_grid.insert({k.pt.x, k.pt.y});
    for (const Point2f &p : b2)
        if (!on_grid.count({p.x, p.y}))
            FAIL("flag off: (%g, %g) is no grid point", p.x, p.y);

    // the extractor by itself
    visualSLAM on;
    configure(on, argv);
    on.FAST_FLAG = true;
    on.fastThreshold = thr;
    std::vector<KeyPoint> fast = on.fastKeypointExtractor(left);
    if (fast.size() < 8)
        FAIL("only %zu FAST key points", fast.size());
    std::set<std::pair<float, float>> corners;
    for (size_t i = 0; i < fast.size(); i++) {
        const KeyPoint &k = fast[i];
        if (k.size != 7.f || k.angle != -1.f || k.response < 1.f)
            FAIL("key point %zu: size %g angle %g response %g", i, k.size, k.angle, k.response);
        if (i && !(k.pt.y > fast[i - 1].pt.y || (k.pt.y == fast[i - 1].pt.y && k.pt.x > fast[i - 1].pt.x)))
            FAIL("key point %zu is out of row-major order", i);
        corners.insert({k.pt.x, k.pt.y});
    }
    print_kps("fast", fast);
    on.fastKeep = keep;
    std::vector<KeyPoint> kept = on.fastKeypointExtractor(left);
    if (kept.empty() || kept.size() > fast.size())
        FAIL("ANMS kept %zu of %zu", kept.size(), fast.size());
    for (size_t i = 0; i < kept.size(); i++) {
        if (!corners.count({kept[i].pt.x, kept[i].pt.y}))
            FAIL("ANMS key point %zu is none of the detector's", i);
        if (i && kept[i].response > kept[i - 1].response)
            FAIL("ANMS key point %zu is out of response order", i);
    }
    print_kps("anms", kept);

    // flag on: reference points from the extractor, then the same LK -> FmatThresholding -> triangulation
    for (int pass = 0; pass < 2; pass++) {
        on.fastKeep = pass ? keep : 0;
        std::set<std::pair<float, float>> src;
        for (const KeyPoint &k : pass ? kept : fast)
            src.insert({k.pt.x, k.pt.y});
        std::vector<Point3f> p3;
        std::vector<Point2f> p2;
        on.stereoTriangulate(left, right, p3, p2);
        if (p2.size() < 8 || p3.size() != p2.size() || on.colors.size() != p2.size())
            FAIL("flag on, pass %d: %zu reference points, %zu 3-D points", pass, p2.size(), p3.size());
        std::printf("# on%d %zu\n", pass, p2.size());
        for (size_t i = 0; i < p2.size(); i++) {
            std::printf("%.9g %.9g %.9g %.9g %.9g\n", p2[i].x, p2[i].y, p3[i].x, p3[i].y, p3[i].z);
            if (!src.count({p2[i].x, p2[i].y}))
                FAIL("flag on, pass %d: reference point %zu (%g, %g) is no FAST key point", pass, i, p2[i].x, p2[i].y);
            if (!(p3[i].z > 0.f))
                FAIL("flag on, pass %d: point %zu has depth %g", pass, i, p3[i].z);
        }
    }
    std::printf("fast anms smoke ok\n");
    return 0;
}
