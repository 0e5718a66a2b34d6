// se3_solve.hip.h -- the per-thread SE(3) and Schur algebra that both bundle adjusters (ba.hip, ba_window.hip) run.  A header of
// its own and not part of small_solve.hip.h: pnp.hip takes chol6_solve from there and needs none of this.
// Every function is held to a checker bit for bit or to 1e-9 (oracle/ba.c, tests/ba_window_numpy.py) and the library is built
// with -ffp-contract=off: the ORDER OF OPERATIONS of each body is its contract.  Do not reassociate, hoist or fuse anything here.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/svo_math.h"  // svo_sin / svo_cos, shared with the oracle

namespace svo {

// Vi = (Hll + lambda I)^-1 by cofactors; Hll and Vi packed symmetric 3 x 3 (00 01 02 11 12 22).  ba_3d2d_kernel (both passes),
// bw_schur_kernel, bw_backsub_kernel.
__device__ __forceinline__ void sym3_inv_damped(const double *Hll, double lambda, double *Vi)
{
    const double a = Hll[0] + lambda, b = Hll[1], c = Hll[2], d = Hll[3] + lambda, e = Hll[4], g = Hll[5] + lambda;
    const double c00 = d * g - e * e, c01 = c * e - b * g, c02 = b * e - c * d;
    const double det = a * c00 + b * c01 + c * c02;
    const double id = 1. / det;
    Vi[0] = c00 * id;
    Vi[1] = c01 * id;
    Vi[2] = c02 * id;
    Vi[3] = (a * g - c * c) * id;
    Vi[4] = (b * c - a * e) * id;
    Vi[5] = (a * d - b * b) * id;
}

// Y = Hpl Vi: 6 x 3 row-major times packed symmetric 3 x 3, every sum left to right.  Pass 1 of ba_3d2d_kernel, bw_schur_kernel.
__device__ __forceinline__ void sym3_mul_rows6(const double *Hpl, const double *Vi, double *Y)
{
#pragma unroll
    for (int r = 0; r < 6; r++) {
        const double *h = Hpl + 3 * r;
        Y[3 * r] = h[0] * Vi[0] + h[1] * Vi[1] + h[2] * Vi[2];
        Y[3 * r + 1] = h[0] * Vi[1] + h[1] * Vi[3] + h[2] * Vi[4];
        Y[3 * r + 2] = h[0] * Vi[2] + h[1] * Vi[4] + h[2] * Vi[5];
    }
}

// out = Vi r (the points' back-substitution): pass 2 of ba_3d2d_kernel, bw_backsub_kernel
__device__ __forceinline__ void sym3_mul_vec(const double *Vi, const double *r3, double *out)
{
    out[0] = Vi[0] * r3[0] + Vi[1] * r3[1] + Vi[2] * r3[2];
    out[1] = Vi[1] * r3[0] + Vi[3] * r3[1] + Vi[4] * r3[2];
    out[2] = Vi[2] * r3[0] + Vi[4] * r3[1] + Vi[5] * r3[2];
}

// (Rn, tn) = SE3Quat::exp([omega; upsilon]) * (R, t), R row-major; tn = (E t) + V upsilon, in that parenthesisation.
// ba_3d2d_kernel, bw_solve_kernel (its poses are stored R9 | t3: it passes P, P + 9).
__device__ inline void se3_exp_mul(const double *d, const double *R, const double *t, double *Rn, double *tn)
{
    const double wx = d[0], wy = d[1], wz = d[2];
    const double th = sqrt(wx * wx + wy * wy + wz * wz);
    const double O[9] = {0, -wz, wy, wz, 0, -wx, -wy, wx, 0};
    double O2[9], E[9], V[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
            O2[3 * i + j] = O[3 * i] * O[j] + O[3 * i + 1] * O[3 + j] + O[3 * i + 2] * O[6 + j];
    if (th < 0.00001) {
        for (int k = 0; k < 9; k++) {
            E[k] = ((k % 4) == 0 ? 1. : 0.) + O[k] + O2[k];
            V[k] = E[k];
        }
    } else {
        const double sn = svo_sin(th), cn = svo_cos(th);
        const double a = sn / th, b = (1. - cn) / (th * th), c = (th - sn) / (th * th * th);
        for (int k = 0; k < 9; k++) {
            const double I = (k % 4) == 0 ? 1. : 0.;
            E[k] = I + a * O[k] + b * O2[k];
            V[k] = I + b * O[k] + c * O2[k];
        }
    }
    double u[3];
    for (int i = 0; i < 3; i++)
        u[i] = V[3 * i] * d[3] + V[3 * i + 1] * d[4] + V[3 * i + 2] * d[5];
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++)
            Rn[3 * i + j] = E[3 * i] * R[j] + E[3 * i + 1] * R[3 + j] + E[3 * i + 2] * R[6 + j];
        tn[i] = (E[3 * i] * t[0] + E[3 * i + 1] * t[1] + E[3 * i + 2] * t[2]) + u[i];
    }
}

// d (u, v) / d pose of the pinhole projection of the camera-frame point (x, y, w), 2 x 6 row-major, [omega; upsilon] ordering
// (g2o types_six_dof_expmap, linearizeOplus).  ba_linearize passes its one focal length twice; bw_linearize builds its stereo row
// from these twelve.
__device__ __forceinline__ void project_pose_jacobian(double x, double y, double w, double fx, double fy, double *B)
{
    const double w2 = w * w;
    B[0] = x * y / w2 * fx;
    B[1] = -(1. + (x * x / w2)) * fx;
    B[2] = y / w * fx;
    B[3] = -1. / w * fx;
    B[4] = 0.;
    B[5] = x / w2 * fx;
    B[6] = (1. + y * y / w2) * fy;
    B[7] = -x * y / w2 * fy;
    B[8] = -x / w * fy;
    B[9] = 0.;
    B[10] = -1. / w * fy;
    B[11] = y / w2 * fy;
}

}  // namespace svo
