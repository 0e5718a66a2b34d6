// StereoProcess with a raw rig through the adaptor, end to end: setCalibration and RECTIFY_FLAG inside stereoMatch,
// reprojectDisparity, stereoTriangulate and monocularTriangulate, the member undistortPoints and the rectification's matrices.
// Usage: rectify_smoke <left pattern> <right pattern> <calib.f64> <out prefix>; the patterns name frame 0 of a raw pair, calib.f64
// holds K1 (9) D1 (4) K2 (9) D2 (4) R (9) T (3) as doubles.
// Writes <prefix>.left / .right (lImg / rImg after stereoMatch: the rectified B,G,R frames), .disp (its int16 map), .xyz / .bgr
// (reprojectDisparity), .pts (four undistorted points of the right camera, float32 pairs) and .mats (R1 R2 P1 P2 Q, 58 doubles).
// Checks in place that RECTIFY_FLAG is off by default, and that stereoTriangulate / monocularTriangulate on the raw frames with the
// flag give what a second adaptor without it gives on the rectified frames.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "svo_compat/stereoCV.hpp"

using namespace svo_compat;

static bool dump(const char *prefix, const char *suffix, const void *p, size_t n)
{
    char path[1024];
    std::snprintf(path, sizeof(path), "%s%s", prefix, suffix);
    FILE *f = std::fopen(path, "wb");
    if (!f)
        return false;
    const bool ok = n == 0 || std::fwrite(p, 1, n, f) == n;
    std::fclose(f);
    return ok;
}

static bool same(const std::vector<Point3f> &a, const std::vector<Point3f> &b)
{
    return a.size() == b.size() && (a.empty() || !std::memcmp(a.data(), b.data(), a.size() * sizeof(Point3f)));
}

// one member call, its outcome as text ("" = returned)
template <class F> static std::string outcome(F &&f)
{
    try {
        f();
    } catch (const std::exception &e) {
        return e.what();
    }
    return "";
}

int main(int argc, char **argv)
{
    if (argc != 5)
        return 2;
    double cal[38];
    FILE *f = std::fopen(argv[3], "rb");
    if (!f || std::fread(cal, sizeof(double), 38, f) != 38)
        return 3;
    std::fclose(f);
    auto vec = [&](int at, int n) { return std::vector<double>(cal + at, cal + at + n); };

    StereoProcess sp(argv[1], argv[2]);
    if (sp.RECTIFY_FLAG)
        return 4;
    sp.setCalibration(vec(0, 9), vec(9, 4), vec(13, 9), vec(22, 4), vec(26, 9), vec(35, 3));
    sp.RECTIFY_FLAG = true;

    // stereoMatch: lImg / rImg become the rectified frames, the map is theirs
    Mat disp = sp.stereoMatch(0);
    if (disp.empty() || sp.lImg.rows != disp.rows || sp.lImg.cols != disp.cols)
        return 5;
    const int w = disp.cols, h = disp.rows;
    if (!dump(argv[4], ".left", sp.lImg.data, (size_t)w * h * 3) || !dump(argv[4], ".right", sp.rImg.data, (size_t)w * h * 3) ||
        !dump(argv[4], ".disp", disp.data, (size_t)w * h * 2))
        return 6;
    // reprojectDisparity: Q of the rig, disparities / 16
    std::vector<Point3f> xyz, bgr;
    sp.reprojectDisparity(disp, xyz, bgr);
    if (!dump(argv[4], ".xyz", xyz.data(), xyz.size() * sizeof(Point3f)) || !dump(argv[4], ".bgr", bgr.data(), bgr.size() * sizeof(Point3f)))
        return 7;

    // the sparse members on the raw frames with the flag == a plain adaptor on the rectified frames
    Mat rawL = sp.getImg(argv[1], 0), rawR = sp.getImg(argv[2], 0);
    StereoProcess plain(argv[1], argv[2]);
    for (StereoProcess *p : {&sp, &plain}) {
        p->focal_x = sp.rectP1[0], p->focal_y = sp.rectP1[5], p->cx = sp.rectP1[2], p->cy = sp.rectP1[6];
        p->baseline = -sp.rectP2[3] / sp.rectP2[0];
    }
    std::vector<Point3f> a, b, ma, mb;
    const std::string oa = outcome([&] { sp.stereoTriangulate(rawL, rawR, a); });
    const std::string ob = outcome([&] { plain.stereoTriangulate(sp.lImg, sp.rImg, b); });
    if (oa != ob || !same(a, b))
        return 8;
    Mat monoL, monoR;
    sp.rectifyPair(rawL, rawR, monoL, monoR, true);  // both through the LEFT camera's map, as monocularTriangulate takes them
    const std::string oma = outcome([&] { sp.monocularTriangulate(rawL, rawR, ma); });
    const std::string omb = outcome([&] { plain.monocularTriangulate(monoL, monoR, mb); });
    if (oma != omb || !same(ma, mb))
        return 9;

    const std::vector<Point2f> pts = {Point2f(10.f, 20.f), Point2f(300.5f, 150.25f), Point2f(158.f, 101.f), Point2f(0.f, 199.f)};
    std::vector<Point2f> und;
    sp.undistortPoints(pts, und, w, h, true);
    if (und.size() != pts.size() || !dump(argv[4], ".pts", und.data(), und.size() * sizeof(Point2f)))
        return 10;
    double mats[58];
    int k = 0;
    for (double v : sp.rectR1) mats[k++] = v;
    for (double v : sp.rectR2) mats[k++] = v;
    for (double v : sp.rectP1) mats[k++] = v;
    for (double v : sp.rectP2) mats[k++] = v;
    for (double v : sp.rectQ) mats[k++] = v;
    if (!dump(argv[4], ".mats", mats, sizeof(mats)))
        return 11;
    std::printf("rectify smoke ok: %d x %d, %zu points reprojected, stereoTriangulate %zu points (%s), monocularTriangulate %zu (%s)\n", w,
                h, xyz.size(), a.size(), oa.empty() ? "returned" : oa.c_str(), ma.size(), oma.empty() ? "returned" : oma.c_str());
    return 0;
}
