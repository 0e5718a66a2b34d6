// The host code of csrc/homography.hip (homography_plan.hip.h) on its own, built with -fsanitize=address,undefined: the
// Jacobi eigen-solver at both of its sizes, checkSubset on hand-made samples, and the decomposition against its definition
// Hn = R + t n^T on planes at several tilts, the pure rotation, singular and extreme input.  Prints one line per
// decomposition ("sol k R.. t.. n..", 17 digits) for a fixed H, which tests/test_homography_abi.py compares with the
// library's answer, then "homography plan check ok".
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "../../ros_stereo_slam_amd/csrc/homography_plan.hip.h"

#define REQUIRE(cond)                                                     \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::printf("%s:%d failed: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                     \
        }                                                                 \
    } while (0)

static const double K4[4] = {718.856, 718.856, 607.1928, 185.2157};

// K (R + t n^T) K^-1
static void pixel_h(const double (&R)[3][3], const double (&t)[3], const double (&n)[3], double *H9)
{
    const double K[3][3] = {{K4[0], 0, K4[2]}, {0, K4[1], K4[3]}, {0, 0, 1}};
    const double Ki[3][3] = {{1 / K4[0], 0, -K4[2] / K4[0]}, {0, 1 / K4[1], -K4[3] / K4[1]}, {0, 0, 1}};
    double M[3][3], A[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
            M[i][j] = R[i][j] + t[i] * n[j];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
            A[i][j] = K[i][0] * M[0][j] + K[i][1] * M[1][j] + K[i][2] * M[2][j];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
            H9[3 * i + j] = A[i][0] * Ki[0][j] + A[i][1] * Ki[1][j] + A[i][2] * Ki[2][j];
}

static void rot_yx(double ay, double ax, double (&R)[3][3])
{
    const double cy = std::cos(ay), sy = std::sin(ay), cx = std::cos(ax), sx = std::sin(ax);
    const double Ry[3][3] = {{cy, 0, sy}, {0, 1, 0}, {-sy, 0, cy}}, Rx[3][3] = {{1, 0, 0}, {0, cx, -sx}, {0, sx, cx}};
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
            R[i][j] = Ry[i][0] * Rx[0][j] + Ry[i][1] * Rx[1][j] + Ry[i][2] * Rx[2][j];
}

int main()
{
    using namespace hm_plan;
    // ---- Jacobi: A = V D V^T, V orthonormal, at 3 and 9 ----
    {
        double A[9][9], A0[9][9], V[9][9];
        unsigned s = 12345;
        for (int i = 0; i < 9; i++)
            for (int j = i; j < 9; j++) {
                s = s * 1664525u + 1013904223u;
                A[i][j] = A[j][i] = A0[i][j] = A0[j][i] = (double)(s >> 8) / (1 << 24) - 0.5;
            }
        jacobi_sym<9>(A, V);
        for (int i = 0; i < 9; i++)
            for (int j = 0; j < 9; j++) {
                double r = 0, o = 0;
                for (int k = 0; k < 9; k++) {
                    r += V[i][k] * A[k][k] * V[j][k];
                    o += V[k][i] * V[k][j];
                }
                REQUIRE(std::fabs(r - A0[i][j]) < 1e-13 && std::fabs(o - (i == j)) < 1e-13);
            }
        double Z[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, VZ[3][3];
        jacobi_sym<3>(Z, VZ);  // nothing to rotate
        REQUIRE(VZ[0][0] == 1 && VZ[1][1] == 1 && VZ[2][2] == 1 && VZ[0][1] == 0);
    }
    // ---- checkSubset ----
    {
        const double sq[4][2] = {{0, 0}, {10, 0}, {10, 10}, {0, 10}}, mv[4][2] = {{3, 3}, {13, 3}, {13, 13}, {3, 13}};
        const double col[4][2] = {{0, 0}, {10, 0}, {20, 0}, {0, 10}}, cross[4][2] = {{0, 0}, {10, 0}, {10, 10}, {5, -4}};
        const double same[4][2] = {{7, 7}, {7, 7}, {7, 7}, {7, 7}};
        REQUIRE(check_subset(sq, mv) && check_subset(cross, cross));
        REQUIRE(!check_subset(col, sq) && !check_subset(sq, col) && !check_subset(sq, cross) && !check_subset(cross, sq));
        REQUIRE(!check_subset(same, same));
    }
    // ---- the decomposition ----
    const double normals[4][3] = {{0, 0, 1}, {0.1, -0.25, 1}, {0.5, 0.1, 1}, {-0.3, 0.6, 1}};
    const double ts[4][3] = {{0.6, -0.1, 0.4}, {0.0, 0.0, 0.5}, {-0.3, 0.2, 0.0}, {0.05, 0.02, -0.2}};
    double R0[3][3];
    rot_yx(-0.05, 0.02, R0);
    for (int a = 0; a < 4; a++)
        for (int b = 0; b < 4; b++) {
            double n[3], nn = std::sqrt(normals[a][0] * normals[a][0] + normals[a][1] * normals[a][1] + normals[a][2] * normals[a][2]);
            for (int k = 0; k < 3; k++)
                n[k] = normals[a][k] / nn;
            const double t[3] = {ts[b][0] / 8, ts[b][1] / 8, ts[b][2] / 8};
            double H9[9], R[36], T[12], N[12];
            pixel_h(R0, t, n, H9);
            REQUIRE(decompose(H9, K4, R, T, N) == 4);
            double best = 1e300;
            for (int k = 0; k < 4; k++) {
                const double *r = R + 9 * k, *tt = T + 3 * k, *nk = N + 3 * k;
                const double det = r[0] * (r[4] * r[8] - r[5] * r[7]) - r[1] * (r[3] * r[8] - r[5] * r[6]) + r[2] * (r[3] * r[7] - r[4] * r[6]);
                REQUIRE(std::fabs(det - 1) < 1e-12 && std::fabs(nk[0] * nk[0] + nk[1] * nk[1] + nk[2] * nk[2] - 1) < 1e-12);
                double e = 0;
                for (int i = 0; i < 3; i++) {
                    for (int j = 0; j < 3; j++)
                        e = std::fmax(e, std::fabs(r[3 * i + j] - R0[i][j]));
                    e = std::fmax(e, std::fmax(std::fabs(tt[i] - t[i]), std::fabs(nk[i] - n[i])));
                }
                best = std::fmin(best, e);
                if (k % 2 == 0) {
                    REQUIRE(nk[2] > 0);
                    for (int i = 0; i < 3; i++)
                        REQUIRE(T[3 * k + i] == -T[3 * (k + 1) + i] && N[3 * k + i] == -N[3 * (k + 1) + i]);
                }
            }
            REQUIRE(best < 1e-6);
            REQUIRE(normal_before(N, N + 6));
            if (a == 2 && b == 0)
                for (int k = 0; k < 4; k++) {
                    std::printf("sol %d", k);
                    for (int i = 0; i < 9; i++)
                        std::printf(" %.17g", R[9 * k + i]);
                    for (int i = 0; i < 3; i++)
                        std::printf(" %.17g", T[3 * k + i]);
                    for (int i = 0; i < 3; i++)
                        std::printf(" %.17g", N[3 * k + i]);
                    std::printf("\n");
                }
        }
    {
        double H9[9], R[36], T[12], N[12];
        const double zero[3] = {0, 0, 0}, ez[3] = {0, 0, 1};
        pixel_h(R0, zero, ez, H9);
        REQUIRE(decompose(H9, K4, R, T, N) == 1 && T[0] == 0 && T[1] == 0 && T[2] == 0 && N[2] == 1);
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++)
                REQUIRE(std::fabs(R[3 * i + j] - R0[i][j]) < 1e-12);
        for (int k = 9; k < 36; k++)
            REQUIRE(R[k] == 0);
        const double none[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, rank1[9] = {1, 1, 1, 2, 2, 2, 3, 3, 3};
        const double huge[9] = {1e300, 0, 0, 0, 1e300, 0, 0, 0, 1e300}, tiny[9] = {1e-200, 0, 0, 0, 1e-200, 0, 0, 0, 1e-200};
        REQUIRE(decompose(none, K4, R, T, N) == 0 && decompose(rank1, K4, R, T, N) == 0);
        REQUIRE(decompose(huge, K4, R, T, N) == 0);  // det overflows: refused, nothing read out of bounds
        const int nt = decompose(tiny, K4, R, T, N);
        REQUIRE(nt == 0 || nt == 1);
        for (int k = 0; k < 36; k++)
            REQUIRE(nt == 1 || R[k] == 0);
    }
    std::printf("homography plan check ok\n");
    return 0;
}
