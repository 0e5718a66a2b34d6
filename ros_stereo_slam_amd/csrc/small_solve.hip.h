// small_solve.hip.h -- small dense solves that more than one kernel file runs per thread.
#pragma once
#include <hip/hip_runtime.h>

namespace svo {

// x = A^-1 b for a symmetric positive definite 6 x 6 A (row-major, lower triangle read) by Cholesky in a fixed order;
// false when a pivot is not positive (NaN included), x then undefined.  oracle/ba.c and oracle/pnp.c run the same steps.
__device__ inline bool chol6_solve(const double *Ain, const double *b, double *x)
{
    double L[36];
    for (int i = 0; i < 36; i++)
        L[i] = 0;
    for (int i = 0; i < 6; i++)
        for (int j = 0; j <= i; j++) {
            double s = Ain[6 * i + j];
            for (int k = 0; k < j; k++)
                s -= L[6 * i + k] * L[6 * j + k];
            if (i == j) {
                if (!(s > 0))
                    return false;
                L[6 * i + i] = sqrt(s);
            } else
                L[6 * i + j] = s / L[6 * j + j];
        }
    double y[6];
    for (int i = 0; i < 6; i++) {
        double s = b[i];
        for (int k = 0; k < i; k++)
            s -= L[6 * i + k] * y[k];
        y[i] = s / L[6 * i + i];
    }
    for (int i = 5; i >= 0; i--) {
        double s = y[i];
        for (int k = i + 1; k < 6; k++)
            s -= L[6 * k + i] * x[k];
        x[i] = s / L[6 * i + i];
    }
    return true;
}

}  // namespace svo
