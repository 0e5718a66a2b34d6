// dlt.hip.h -- the DLT triangulation's 4 x 4 solver, shared by geometry.hip (cv::triangulatePoints), essential.hip
// (recoverPose's cheirality test) and homography.hip (the same test on the candidates of a decomposed H).
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>

namespace svo {

// right singular vector of the smallest singular value of a 4x4 matrix (Hestenes Jacobi)
__device__ inline void smallest_right_singular_vector4(double (&A)[4][4], double (&v)[4])
{
    double V[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++)
            V[i][j] = i == j ? 1. : 0.;
    for (int sweep = 0; sweep < 30; sweep++) {
        bool rotated = false;
#pragma unroll
        for (int p = 0; p < 3; p++)
#pragma unroll
            for (int q = p + 1; q < 4; q++) {
                double al = 0, be = 0, ga = 0;
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    al += A[i][p] * A[i][p];
                    be += A[i][q] * A[i][q];
                    ga += A[i][p] * A[i][q];
                }
                if (fabs(ga) <= DBL_EPSILON * sqrt(al * be) || ga == 0)
                    continue;
                rotated = true;
                const double zeta = (be - al) / (2. * ga);
                const double t = (zeta >= 0 ? 1. : -1.) / (fabs(zeta) + sqrt(1. + zeta * zeta));
                const double c = 1. / sqrt(1. + t * t), s = c * t;
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const double ap = A[i][p], aq = A[i][q];
                    A[i][p] = c * ap - s * aq;
                    A[i][q] = s * ap + c * aq;
                    const double vp = V[i][p], vq = V[i][q];
                    V[i][p] = c * vp - s * vq;
                    V[i][q] = s * vp + c * vq;
                }
            }
        if (!rotated)
            break;
    }
    int best = 0;
    double bn = DBL_MAX;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        double nn = 0;
#pragma unroll
        for (int i = 0; i < 4; i++)
            nn += A[i][j] * A[i][j];
        if (nn < bn) {
            bn = nn;
            best = j;
        }
    }
#pragma unroll
    for (int i = 0; i < 4; i++)
        v[i] = best == 0 ? V[i][0] : best == 1 ? V[i][1] : best == 2 ? V[i][2] : V[i][3];
}

// one point against one candidate P = [R|t] (normalised coordinates): the DLT with P0 = [I|0], then recoverPose's tests
__device__ __forceinline__ bool rp_point_good(const double (&P)[12], double x1, double y1, double x2, double y2, double dist)
{
    const double P0[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    double A[4][4], Q[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        A[0][k] = x1 * P0[8 + k] - P0[k];
        A[1][k] = y1 * P0[8 + k] - P0[4 + k];
        A[2][k] = x2 * P[8 + k] - P[k];
        A[3][k] = y2 * P[8 + k] - P[4 + k];
    }
    smallest_right_singular_vector4(A, Q);
    bool ok = Q[2] * Q[3] > 0;
    const double X = Q[0] / Q[3], Y = Q[1] / Q[3], Z = Q[2] / Q[3], W = Q[3] / Q[3];
    ok = ok && Z < dist;
    const double z2 = P[8] * X + P[9] * Y + P[10] * Z + P[11] * W;
    return ok && z2 > 0 && z2 < dist;
}

}  // namespace svo
