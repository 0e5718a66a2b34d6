// StereoProcess::monocularTriangulate with HOMOGRAPHY_FLAG set, through the adaptor on two frames read from files.
// Usage: homography_mono_smoke <frame1> <frame2> <w> <h> <out prefix>; the frames: h x w x 3 uint8, B,G,R.  Writes
// <prefix>.xyz (out3d, float32 triples), <prefix>.pts (the F-inlier pairs, float32 x1 y1 x2 y2) and <prefix>.pose
// (R row-major, t and the plane's normal, 15 doubles).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "svo_compat/stereoCV.hpp"

using namespace svo_compat;

static bool read_all(const char *path, void *p, size_t bytes)
{
    FILE *f = std::fopen(path, "rb");
    if (!f)
        return false;
    const bool ok = std::fread(p, 1, bytes, f) == bytes;
    std::fclose(f);
    return ok;
}

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
    if (argc != 6)
        return 2;
    const int w = std::atoi(argv[3]), h = std::atoi(argv[4]);
    Mat a(h, w, CV_8UC3), b(h, w, CV_8UC3);
    if (!read_all(argv[1], a.data, (size_t)w * h * 3) || !read_all(argv[2], b.data, (size_t)w * h * 3))
        return 3;
    StereoProcess sp;
    sp.HOMOGRAPHY_FLAG = true;
    std::vector<Point3f> out3d;
    sp.monocularTriangulate(a, b, out3d);
    if (out3d.size() != sp.monoPts1.size() || out3d.empty())
        return 4;
    std::vector<float> pts;
    for (size_t i = 0; i < sp.monoPts1.size(); i++) {
        pts.push_back(sp.monoPts1[i].x);
        pts.push_back(sp.monoPts1[i].y);
        pts.push_back(sp.monoPts2[i].x);
        pts.push_back(sp.monoPts2[i].y);
    }
    double pose[15];
    for (int k = 0; k < 9; k++)
        pose[k] = sp.monoR[k];
    for (int k = 0; k < 3; k++) {
        pose[9 + k] = sp.monoT[k];
        pose[12 + k] = sp.planeNormal[k];
    }
    if (!dump(argv[5], ".xyz", out3d.data(), out3d.size() * sizeof(Point3f)) ||
        !dump(argv[5], ".pts", pts.data(), pts.size() * sizeof(float)) || !dump(argv[5], ".pose", pose, sizeof(pose)))
        return 6;
    std::printf("homography mono smoke ok: %zu points\n", out3d.size());
    return 0;
}
