// homography_plan.hip.h -- the parts of homography.hip that need no device and that the host runs too: the symmetric Jacobi
// eigen-solver (3 x 3 here, 9 x 9 in the refit), checkSubset of a 4-sample and cv::decomposeHomographyMat.  Plain C++ apart from
// the __host__ __device__ marks, so tests/cpp/homography_plan_check.cpp builds it alone under the sanitizers.  Every operation
// is one of + - * / sqrt in a stated order: tests/homography_numpy.py restates them one for one.
#pragma once
#include <cfloat>
#include <cmath>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HM_HD __host__ __device__
#else
#define HM_HD
#endif

namespace hm_plan {

constexpr double kPureRotation = 1e-8;  // lambda1 - lambda3 of Hn^T Hn (lambda2 = 1) at or below this: a pure rotation
constexpr int kJacobiSweeps = 30;

// one Jacobi rotation for the pair (p, q) of a symmetric matrix: false when the entry is already negligible
HM_HD inline bool jacobi_angle(double app, double aqq, double apq, double &c, double &s)
{
    if (apq == 0 || fabs(apq) <= DBL_EPSILON * sqrt(fabs(app * aqq)))
        return false;
    const double theta = (aqq - app) / (2. * apq);
    const double t = (theta >= 0 ? 1. : -1.) / (fabs(theta) + sqrt(theta * theta + 1.));
    c = 1. / sqrt(t * t + 1.);
    s = c * t;
    return true;
}

// A = V diag(A) V^T: cyclic Jacobi, pairs (0,1), (0,2) .. (N-2,N-1); per pair the columns p, q of every row, then the rows
// p, q of every column, then the columns of V.  A is overwritten (its diagonal: the eigenvalues, unordered).
template <int N> HM_HD inline void jacobi_sym(double (&A)[N][N], double (&V)[N][N])
{
    for (int i = 0; i < N; i++)
        for (int j = 0; j < N; j++)
            V[i][j] = i == j ? 1. : 0.;
    for (int sweep = 0; sweep < kJacobiSweeps; sweep++) {
        bool rotated = false;
        for (int p = 0; p < N - 1; p++)
            for (int q = p + 1; q < N; q++) {
                double c, s;
                if (!jacobi_angle(A[p][p], A[q][q], A[p][q], c, s))
                    continue;
                rotated = true;
                for (int k = 0; k < N; k++) {
                    const double ap = A[k][p], aq = A[k][q];
                    A[k][p] = c * ap - s * aq;
                    A[k][q] = s * ap + c * aq;
                }
                for (int k = 0; k < N; k++) {
                    const double ap = A[p][k], aq = A[q][k];
                    A[p][k] = c * ap - s * aq;
                    A[q][k] = s * ap + c * aq;
                }
                for (int k = 0; k < N; k++) {
                    const double vp = V[k][p], vq = V[k][q];
                    V[k][p] = c * vp - s * vq;
                    V[k][q] = s * vp + c * vq;
                }
            }
        if (!rotated)
            break;
    }
}

// twice the signed area of the triple (i, j, k) and the collinearity test of cv haveCollinearPoints on it
HM_HD inline double triple_cross(const double (&p)[4][2], int i, int j, int k, bool &collinear)
{
    const double dx1 = p[j][0] - p[i][0], dy1 = p[j][1] - p[i][1], dx2 = p[k][0] - p[i][0], dy2 = p[k][1] - p[i][1];
    const double c = dx1 * dy2 - dy1 * dx2;
    collinear = fabs(c) <= (double)FLT_EPSILON * (fabs(dx1) + fabs(dy1) + fabs(dx2) + fabs(dy2));
    return c;
}

// HomographyEstimatorCallback::checkSubset on a 4-sample: no triple collinear in either image, every triple turning the
// same way in both
HM_HD inline bool check_subset(const double (&a)[4][2], const double (&b)[4][2])
{
    const int tt[4][3] = {{0, 1, 2}, {1, 2, 3}, {0, 2, 3}, {0, 1, 3}};
    bool ok = true;
    for (int m = 0; m < 4; m++) {
        bool la, lb;
        const double ca = triple_cross(a, tt[m][0], tt[m][1], tt[m][2], la);
        const double cb = triple_cross(b, tt[m][0], tt[m][1], tt[m][2], lb);
        ok = ok && !la && !lb && ((ca > 0) == (cb > 0));
    }
    return ok;
}

HM_HD inline void cross3(const double *a, const double *b, double *c)
{
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// (nz, ny, nx) of a before that of b in descending lexicographic order
HM_HD inline bool normal_before(const double *a, const double *b)
{
    if (a[2] != b[2])
        return a[2] > b[2];
    if (a[1] != b[1])
        return a[1] > b[1];
    return a[0] >= b[0];
}

// cv::decomposeHomographyMat, by the eigen-decomposition of Hn^T Hn (Faugeras / Zhang, as Ma, Soatto, Kosecka, Sastry
// state it): Hn = K^-1 H K, its sign chosen so that det Hn > 0, scaled so that its middle singular value is 1;
// lambda1 >= 1 >= lambda3 and v1, v2, v3 the eigen-pairs of Hn^T Hn;
//   u = (sqrt(1 - lambda3) v1 +- sqrt(lambda1 - 1) v3) / sqrt(lambda1 - lambda3)
//   U = [v2, u, v2 x u], W = [Hn v2, Hn u, Hn v2 x Hn u], R = W U^T, n = v2 x u, t = (Hn - R) n
// so that Hn = R + t n^T.  Of (t, n) and (-t, -n) the first has nz > 0 (nz = 0: ny > 0; then nx > 0).  Of the two
// solutions `a` is the one whose first normal comes first by (nz, ny, nx) descending.  Order: (Ra, ta, na),
// (Ra, -ta, -na), (Rb, tb, nb), (Rb, -tb, -nb).  lambda1 - lambda3 <= kPureRotation: one solution, R the rotation nearest
// Hn, t = 0, n = (0, 0, 1).  Returns the number of solutions (0: H is singular or not finite).  R: 4 x 9, t, n: 4 x 3.
HM_HD inline int decompose(const double *H9, const double *K4, double *R, double *t, double *n)
{
    for (int k = 0; k < 36; k++)
        R[k] = 0;
    for (int k = 0; k < 12; k++)
        t[k] = n[k] = 0;
    const double fx = K4[0], fy = K4[1], cx = K4[2], cy = K4[3];
    double A[3][3], H[3][3];
    for (int i = 0; i < 3; i++) {
        A[i][0] = H9[3 * i] * fx;
        A[i][1] = H9[3 * i + 1] * fy;
        A[i][2] = H9[3 * i] * cx + H9[3 * i + 1] * cy + H9[3 * i + 2];
    }
    for (int j = 0; j < 3; j++) {
        H[0][j] = (A[0][j] - cx * A[2][j]) / fx;
        H[1][j] = (A[1][j] - cy * A[2][j]) / fy;
        H[2][j] = A[2][j];
    }
    const double det = H[0][0] * (H[1][1] * H[2][2] - H[1][2] * H[2][1]) - H[0][1] * (H[1][0] * H[2][2] - H[1][2] * H[2][0]) +
                       H[0][2] * (H[1][0] * H[2][1] - H[1][1] * H[2][0]);
    if (!(fabs(det) > 0) || !std::isfinite(det))
        return 0;
    double S[3][3], V[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = i; j < 3; j++)
            S[i][j] = S[j][i] = H[0][i] * H[0][j] + H[1][i] * H[1][j] + H[2][i] * H[2][j];
    jacobi_sym<3>(S, V);
    int o[3] = {0, 1, 2};
    for (int i = 1; i < 3; i++)
        for (int j = i; j > 0 && S[o[j]][o[j]] > S[o[j - 1]][o[j - 1]]; j--) {
            const int x = o[j];
            o[j] = o[j - 1];
            o[j - 1] = x;
        }
    const double l2 = S[o[1]][o[1]];
    if (!(l2 > 0) || !std::isfinite(l2))
        return 0;
    const double sc = (det < 0 ? -1. : 1.) / sqrt(l2);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
            H[i][j] *= sc;
    const double l1 = S[o[0]][o[0]] / l2, l3 = S[o[2]][o[2]] / l2;
    double v1[3], v2[3], v3[3];
    for (int i = 0; i < 3; i++) {
        v1[i] = V[i][o[0]];
        v2[i] = V[i][o[1]];
        v3[i] = V[i][o[2]];
    }
    if (!(l3 > 0) || !std::isfinite(l1))
        return 0;
    if (l1 - l3 <= kPureRotation) {
        // R = Hn V diag(lambda^-1/2) V^T
        const double w[3] = {1. / sqrt(l1), 1., 1. / sqrt(l3)};
        const double *v[3] = {v1, v2, v3};
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) {
                double r = 0;
                for (int m = 0; m < 3; m++) {
                    const double hv = H[i][0] * v[m][0] + H[i][1] * v[m][1] + H[i][2] * v[m][2];
                    r += hv * w[m] * v[m][j];
                }
                R[3 * i + j] = r;
            }
        n[2] = 1.;
        return 1;
    }
    const double ca = sqrt(1. - l3 > 0 ? 1. - l3 : 0.), cb = sqrt(l1 - 1. > 0 ? l1 - 1. : 0.), den = sqrt(l1 - l3);
    double Rs[2][9], ts[2][3], ns[2][3];
    for (int m = 0; m < 2; m++) {
        const double sg = m == 0 ? 1. : -1.;
        double u[3], N[3], hv[3], hu[3], hn[3];
        for (int i = 0; i < 3; i++)
            u[i] = (ca * v1[i] + sg * cb * v3[i]) / den;
        cross3(v2, u, N);
        for (int i = 0; i < 3; i++) {
            hv[i] = H[i][0] * v2[0] + H[i][1] * v2[1] + H[i][2] * v2[2];
            hu[i] = H[i][0] * u[0] + H[i][1] * u[1] + H[i][2] * u[2];
        }
        cross3(hv, hu, hn);
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++)
                Rs[m][3 * i + j] = hv[i] * v2[j] + hu[i] * u[j] + hn[i] * N[j];
        const bool flip = N[2] != 0 ? N[2] < 0 : (N[1] != 0 ? N[1] < 0 : N[0] < 0);
        for (int i = 0; i < 3; i++) {
            const double T = (H[i][0] - Rs[m][3 * i]) * N[0] + (H[i][1] - Rs[m][3 * i + 1]) * N[1] + (H[i][2] - Rs[m][3 * i + 2]) * N[2];
            ts[m][i] = flip ? -T : T;
        }
        for (int i = 0; i < 3; i++)
            ns[m][i] = flip ? -N[i] : N[i];
    }
    const int a = normal_before(ns[0], ns[1]) ? 0 : 1;
    for (int m = 0; m < 2; m++) {
        const int src = m == 0 ? a : 1 - a;
        for (int k = 0; k < 9; k++)
            R[(2 * m) * 9 + k] = R[(2 * m + 1) * 9 + k] = Rs[src][k];
        for (int k = 0; k < 3; k++) {
            t[(2 * m) * 3 + k] = ts[src][k];
            t[(2 * m + 1) * 3 + k] = -ts[src][k];
            n[(2 * m) * 3 + k] = ns[src][k];
            n[(2 * m + 1) * 3 + k] = -ns[src][k];
        }
    }
    return 4;
}

}  // namespace hm_plan
