// visualOdometry::BundleAdjustWindow (svo_ba_window behind the adaptor's types) on a window of three poses.
//   ba_window_smoke            a built-in window: 60 points seen by all three poses (the first held, stereo there, mono elsewhere);
//                              checks that chi2 falls, that the held pose is untouched and that the free poses move towards the truth.
//   ba_window_smoke <file>     the window of a text file (written by tests/test_gpu_ba_window.py; numbers as C hex floats):
//                              "P N M iterations", "fx fy cx cy bf huber_mono huber_stereo", P lines of 12 pose numbers and a flag,
//                              N lines "x y z", N + 1 starts, M lines "pose u v ur".
// Either way it prints the refined poses, one "pose j" line of 12 hex floats each, the six info values and "ba window smoke ok".
#include <cmath>
#include <cstdio>
#include <vector>

#include "svo_compat/bundleAdjust.hpp"

using namespace svo_compat;

#define FAIL(...)                          \
    do {                                   \
        std::fprintf(stderr, __VA_ARGS__); \
        std::fprintf(stderr, "\n");        \
        return 1;                          \
    } while (0)

int main(int argc, char **argv)
{
    int P = 3, N = 60, M = 0, iterations = 10;
    double cam[7] = {718.856, 700.0, 607.1928, 185.2157, 718.856 * 0.54, 0, 0};
    std::vector<double> poses, truth;
    std::vector<unsigned char> fixed;
    std::vector<Point3f> pts;
    std::vector<int> start, pose;
    std::vector<float> uvr;
    if (argc > 1) {
        FILE *f = std::fopen(argv[1], "r");
        if (!f)
            FAIL("cannot open %s", argv[1]);
        if (std::fscanf(f, "%d %d %d %d", &P, &N, &M, &iterations) != 4 || P < 1 || N < 1 || M < 0)
            FAIL("bad header");
        for (double &c : cam)
            if (std::fscanf(f, "%la", &c) != 1)
                FAIL("bad camera line");
        poses.resize(12 * (size_t)P);
        fixed.resize(P);
        for (int j = 0; j < P; j++) {
            int flag;
            for (int k = 0; k < 12; k++)
                if (std::fscanf(f, "%la", &poses[12 * j + k]) != 1)
                    FAIL("bad pose line");
            if (std::fscanf(f, "%d", &flag) != 1)
                FAIL("bad pose flag");
            fixed[j] = (unsigned char)flag;
        }
        for (int i = 0; i < N; i++) {
            double x, y, z;
            if (std::fscanf(f, "%la %la %la", &x, &y, &z) != 3)
                FAIL("bad point line");
            pts.emplace_back((float)x, (float)y, (float)z);
        }
        start.resize(N + 1);
        for (int &s : start)
            if (std::fscanf(f, "%d", &s) != 1)
                FAIL("bad start");
        pose.resize(M);
        uvr.resize(3 * (size_t)M);
        for (int o = 0; o < M; o++) {
            double u, v, r;
            if (std::fscanf(f, "%d %la %la %la", &pose[o], &u, &v, &r) != 4)
                FAIL("bad observation line");
            uvr[3 * o] = (float)u;
            uvr[3 * o + 1] = (float)v;
            uvr[3 * o + 2] = (float)r;
        }
        std::fclose(f);
    } else {
        unsigned lcg = 2024;
        auto rnd = [&]() {
            lcg = lcg * 1664525u + 1013904223u;
            return (double)(lcg >> 8) / (1 << 24);
        };
        for (int j = 0; j < P; j++) {  // the truth: no rotation, the camera advancing 0.35 m a frame
            const double tj[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0.03 * j, -0.01 * j, -0.35 * j};
            truth.insert(truth.end(), tj, tj + 12);
        }
        poses = truth;
        for (int j = 1; j < P; j++) {
            poses[12 * j + 9] += 0.05;
            poses[12 * j + 10] -= 0.02;
            poses[12 * j + 11] += 0.04;
        }
        fixed = {1, 0, 0};
        start.push_back(0);
        for (int i = 0; i < N; i++) {
            const double X = -8 + 16 * rnd(), Y = -2 + 4 * rnd(), Z = 6 + 30 * rnd();
            pts.emplace_back((float)(X + 0.1 * (rnd() - 0.5)), (float)(Y + 0.1 * (rnd() - 0.5)), (float)(Z + 0.1 * (rnd() - 0.5)));
            for (int j = 0; j < P; j++) {
                const double x = X + truth[12 * j + 9], y = Y + truth[12 * j + 10], z = Z + truth[12 * j + 11];
                const double u = x / z * cam[0] + cam[2] + 0.4 * (rnd() - 0.5), v = y / z * cam[1] + cam[3] + 0.4 * (rnd() - 0.5);
                pose.push_back(j);
                uvr.push_back((float)u);
                uvr.push_back((float)v);
                uvr.push_back(j == 0 ? (float)(u - cam[4] / z + 0.4 * (rnd() - 0.5)) : std::nanf(""));
            }
            start.push_back((int)pose.size());
        }
        M = (int)pose.size();
    }

    std::vector<Mat> R, t;
    for (int j = 0; j < P; j++) {
        Mat Rj = Mat::zeros(3, 3, CV_64F), tj = Mat::zeros(3, 1, CV_64F);
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++)
                Rj.at<double>(r, c) = poses[12 * j + 3 * r + c];
            tj.at<double>(r, 0) = poses[12 * j + 9 + r];
        }
        R.push_back(Rj);
        t.push_back(tj);
    }
    Mat K = Mat::zeros(3, 3, CV_64F);
    K.at<double>(0, 0) = cam[0];
    K.at<double>(1, 1) = cam[1];
    K.at<double>(0, 2) = cam[2];
    K.at<double>(1, 2) = cam[3];
    K.at<double>(2, 2) = 1;
    visualOdometry od;
    od.baIterations = iterations;
    od.baWindowHuberMono = cam[5];
    od.baWindowHuberStereo = cam[6];
    std::vector<double> chi2;
    od.BundleAdjustWindow(R, t, fixed, pts, start, pose, uvr, K, cam[4], nullptr, &chi2);
    for (int j = 0; j < P; j++) {
        std::printf("pose %d", j);
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++)
                std::printf(" %a", R[j].at<double>(r, c));
        for (int r = 0; r < 3; r++)
            std::printf(" %a", t[j].at<double>(r, 0));
        std::printf("\n");
    }
    std::printf("info");
    for (double v : od.lastWindowInfo)
        std::printf(" %a", v);
    std::printf("\n");
    if ((int)chi2.size() != M || od.lastWindowInfo[5] != M)
        FAIL("observation count: %zu chi2 values, info says %g, expected %d", chi2.size(), od.lastWindowInfo[5], M);
    if (argc == 1) {
        if (!(od.lastWindowInfo[1] < od.lastWindowInfo[0]) || !(od.lastWindowInfo[1] > 1e-3 * od.lastWindowInfo[0]))
            FAIL("chi2 %g -> %g: it must fall and must not collapse", od.lastWindowInfo[0], od.lastWindowInfo[1]);
        for (int k = 0; k < 12; k++)
            if ((k < 9 ? R[0].at<double>(k / 3, k % 3) : t[0].at<double>(k - 9, 0)) != truth[k])
                FAIL("the held pose moved");
        for (int j = 1; j < P; j++) {
            double e0 = 0, e1 = 0;
            for (int r = 0; r < 3; r++) {
                e0 += (poses[12 * j + 9 + r] - truth[12 * j + 9 + r]) * (poses[12 * j + 9 + r] - truth[12 * j + 9 + r]);
                e1 += (t[j].at<double>(r, 0) - truth[12 * j + 9 + r]) * (t[j].at<double>(r, 0) - truth[12 * j + 9 + r]);
            }
            if (!(e1 < 0.25 * e0))
                FAIL("pose %d: |t - truth|^2 %g -> %g", j, e0, e1);
        }
    }
    std::printf("ba window smoke ok\n");
    return 0;
}
