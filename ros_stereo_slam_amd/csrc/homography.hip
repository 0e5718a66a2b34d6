// homography.hip -- homography RANSAC, its refit and polish, and the planar two-view pose for gfx950.
//
// Replaces cv::findHomography(p1, p2, RANSAC, threshold, mask, max_iters, confidence) of OpenCV 3.2 (fundam.cpp, ptsetreg.cpp)
// and cv::decomposeHomographyMat followed by a recoverPose-style choice among its candidates.  Up to SVO_LK_MAX_JOBS
// independent problems per call (CSR offsets into one point array), as essential.hip.
//
//   hm_solve    one LANE per RANSAC iteration: the 4-sample (draw_distinct<4>, keyed by (seed, iteration)), checkSubset, a
//               rejected sample drawn again at most kMaxAttempts times (the draw counter carries on, as fr_solve_wave), then
//               the minimal solve; the model goes to HBM
//   hm_score    one WAVE per iteration: the float forward transfer error of every pair, points strided over the lanes, the
//               count reduced exactly as an integer
//   hm_replay   one thread per problem replays the SEQUENTIAL loop over the counts (ransac_replay<1>: first-best-wins,
//               adaptive bound), so the answer is the serial algorithm's whatever the schedule
//   hm_finish   one WORKGROUP per problem: the loop's mask, the refit of the winner over its inliers (normalised DLT), at
//               most ten Levenberg-Marquardt steps, the outputs
// Three phases (iterations [0, 64), [64, 256), [256, max_iters)); a phase whose problem has already stopped leaves at once.
//
// Where OpenCV calls its own linear algebra, this file chooses (tests/homography_numpy.py restates the choices):
//   minimal solve  per-axis normalisation (mean, then 4 / sum |v - mean|, as runKernel), the 8 x 8 system with h8 = 1 in
//                  normalised coordinates by Gaussian elimination with partial pivoting (a pivot at or below 1e-10: no
//                  model), de-normalised, scaled to h8 = 1.  OpenCV takes the 9 x 9 null vector; the two agree whenever
//                  h8 != 0 in normalised coordinates;
//   checkSubset    all four triples are tested for collinearity (OpenCV: the three that hold the last point), and a sample
//                  passes only when every triple turns the same way in both images (OpenCV also passes four flips, a
//                  mirrored plane, which no camera pair produces); a sample still rejected after kMaxAttempts draws makes
//                  its iteration score no model (OpenCV's getSubset gives up after 1000 draws and ends the loop);
//   refit          L^T L (45 sums) through block_sum: thread t adds the inliers t, t + 256, .. in order, then the fixed
//                  tree; the eigenvector of the smallest eigenvalue by cyclic Jacobi (homography_plan.hip.h); no sign rule
//                  is needed, H is scaled to h8 = 1;
//   polish         HomographyRefineCallback's residuals and Jacobian on h0 .. h7; lambda starts at 1e-3; a step solves
//                  (J^T J + lambda diag(J^T J)) d = -J^T r by Cholesky; it is taken when the cost falls (lambda / 10) and
//                  dropped otherwise (lambda * 10); at most ten steps; stops early when max |d| <= 1e-12 max(1, max |h|) or
//                  the factorisation fails.  (OpenCV's LMSolver keeps another schedule for lambda.)
// The mask is the loop's, not recomputed after the polish, as upstream.
#include <cfloat>
#include <cmath>

#include "dlt.hip.h"
#include "homography_plan.hip.h"
#include "ransac_common.hip.h"
#include "svo_internal.h"

using namespace svo;

namespace {

constexpr int MP = 4;  // model points
constexpr int MAX_ITERS = 20000;
constexpr int LM_STEPS = 10;

// one axis of four values: its mean c and s = 4 / sum |v - c|; false when the spread vanishes
__device__ __forceinline__ bool hm_axis4(const double (&p)[4][2], int ax, double &c, double &s)
{
    c = (((p[0][ax] + p[1][ax]) + p[2][ax]) + p[3][ax]) / 4.;
    const double d = ((fabs(p[0][ax] - c) + fabs(p[1][ax] - c)) + fabs(p[2][ax] - c)) + fabs(p[3][ax] - c);
    if (!(d >= DBL_EPSILON))
        return false;
    s = 4. / d;
    return true;
}

// H = T2^-1 Hn T1 scaled to h8 = 1, with T1 = [s1 (v - c1)] on image 1 and T2 on image 2; false: h8 = 0 or not finite
__device__ __forceinline__ bool hm_denormalise(const double (&g)[9], const double (&c1)[2], const double (&s1)[2],
                                               const double (&c2)[2], const double (&s2)[2], double (&H)[9])
{
    double T[3][3], G[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        T[i][0] = g[3 * i] * s1[0];
        T[i][1] = g[3 * i + 1] * s1[1];
        T[i][2] = g[3 * i] * (-c1[0] * s1[0]) + g[3 * i + 1] * (-c1[1] * s1[1]) + g[3 * i + 2];
    }
#pragma unroll
    for (int j = 0; j < 3; j++) {
        G[0][j] = T[0][j] / s2[0] + c2[0] * T[2][j];
        G[1][j] = T[1][j] / s2[1] + c2[1] * T[2][j];
        G[2][j] = T[2][j];
    }
    const double w = G[2][2];
    if (!(fabs(w) > 0))
        return false;
    bool fin = true;
#pragma unroll
    for (int k = 0; k < 9; k++) {
        H[k] = G[k / 3][k % 3] / w;
        fin = fin && isfinite(H[k]);
    }
    return fin;
}

// the minimal solver on one 4-sample (the file header): H (h8 = 1) or false
__device__ bool hm_solve4(const double (&a)[4][2], const double (&b)[4][2], double (&H)[9])
{
    if (!hm_plan::check_subset(a, b))
        return false;
    double c1[2], s1[2], c2[2], s2[2];
    if (!hm_axis4(a, 0, c1[0], s1[0]) || !hm_axis4(a, 1, c1[1], s1[1]) || !hm_axis4(b, 0, c2[0], s2[0]) ||
        !hm_axis4(b, 1, c2[1], s2[1]))
        return false;
    double M[8][9];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const double X = (a[i][0] - c1[0]) * s1[0], Y = (a[i][1] - c1[1]) * s1[1];
        const double x = (b[i][0] - c2[0]) * s2[0], y = (b[i][1] - c2[1]) * s2[1];
        const double r0[9] = {X, Y, 1., 0., 0., 0., -x * X, -x * Y, x}, r1[9] = {0., 0., 0., X, Y, 1., -y * X, -y * Y, y};
#pragma unroll
        for (int c = 0; c < 9; c++) {
            M[2 * i][c] = r0[c];
            M[2 * i + 1][c] = r1[c];
        }
    }
#pragma unroll
    for (int k = 0; k < 8; k++) {
        int p = k;
        double best = fabs(M[k][k]);
#pragma unroll
        for (int r = k + 1; r < 8; r++)
            if (fabs(M[r][k]) > best) {
                best = fabs(M[r][k]);
                p = r;
            }
        if (!(best > 1e-10))
            return false;
#pragma unroll
        for (int r = k + 1; r < 8; r++)
            if (r == p) {
#pragma unroll
                for (int c = k; c < 9; c++) {
                    const double tmp = M[k][c];
                    M[k][c] = M[r][c];
                    M[r][c] = tmp;
                }
            }
#pragma unroll
        for (int r = k + 1; r < 8; r++) {
            const double f = M[r][k] / M[k][k];
#pragma unroll
            for (int c = k + 1; c < 9; c++)
                M[r][c] -= f * M[k][c];
        }
    }
    double g[9];
    g[8] = 1.;
#pragma unroll
    for (int k = 7; k >= 0; k--) {
        double acc = M[k][8];
#pragma unroll
        for (int c = k + 1; c < 8; c++)
            acc -= M[k][c] * g[c];
        g[k] = acc / M[k][k];
    }
    return hm_denormalise(g, c1, s1, c2, s2, H);
}

// cv HomographyEstimatorCallback::computeError: float throughout
__device__ __forceinline__ float hm_error(const float (&Hf)[8], float X, float Y, float x, float y)
{
    const float ww = 1.f / (Hf[6] * X + Hf[7] * Y + 1.f);
    const float dx = (Hf[0] * X + Hf[1] * Y + Hf[2]) * ww - x;
    const float dy = (Hf[3] * X + Hf[4] * Y + Hf[5]) * ww - y;
    return dx * dx + dy * dy;
}

// pair i of a point array (the arrays of a caller are only known to be float-aligned)
__device__ __forceinline__ float2 hm_pair(const float *p, int i) { return make_float2(p[2 * i], p[2 * i + 1]); }

struct HmJob {
    const float *p1, *p2;  // pixels, n pairs
    int n;
    float thr;             // threshold^2
    RansacState *st;
    double *Hm;            // max_iters x 8 (h8 = 1)
    int *nmodels, *counts; // max_iters each
    uint8_t *mask;
    double *H_out;         // 9
    int *count_out, *iters_out;
};
struct HmBatch {
    HmJob j[SVO_LK_MAX_JOBS];
};
static_assert(sizeof(HmBatch) + 64 <= 4096, "kernel arguments are limited to 4 KB");

// the iterations [it0, lim) a phase still has to run for this problem (lim <= it0: none)
__device__ __forceinline__ int hm_phase_limit(const HmJob &job, int max_iters, int it0, int it1)
{
    const int n = job.n;
    if (n < MP || (n == MP && it0 > 0))
        return 0;
    int lim = it1 < max_iters ? it1 : max_iters;
    if (n == MP)
        return 1;  // exactly four pairs: the solver once, on the pairs as they stand
    if (it0 > 0) {
        const RansacState s = *job.st;  // written by the previous phase's replay
        if (s.done)
            return 0;
        lim = lim < s.niters ? lim : s.niters;
    }
    return lim;
}

__global__ __launch_bounds__(64) void hm_solve_kernel(HmBatch b, uint64_t seed, int max_iters, int it0, int it1)
{
    svo_chain_priority();
    const HmJob &job = b.j[blockIdx.y];
    const int n = job.n, lim = hm_phase_limit(job, max_iters, it0, it1);
    const int it = it0 + (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (it >= lim)
        return;
    int idx[MP] = {0, 1, 2, 3};
    double a[4][2], c[4][2];
    bool drawn = true, ok = false;
    uint32_t draw = 0;
    for (int attempt = 0; attempt < (n == MP ? 1 : kMaxAttempts) && !ok; attempt++) {
        if (n > MP && !draw_distinct(seed, it, n, draw, idx)) {
            drawn = false;
            break;
        }
#pragma unroll
        for (int k = 0; k < MP; k++) {
            a[k][0] = (double)job.p1[2 * idx[k]], a[k][1] = (double)job.p1[2 * idx[k] + 1];
            c[k][0] = (double)job.p2[2 * idx[k]], c[k][1] = (double)job.p2[2 * idx[k] + 1];
        }
        ok = hm_plan::check_subset(a, c);
    }
    double H[9];
    const bool solved = ok && hm_solve4(a, c, H);
    job.nmodels[it] = !drawn ? -1 : (solved ? 1 : 0);
    if (solved)
#pragma unroll
        for (int k = 0; k < 8; k++)
            job.Hm[(size_t)it * 8 + k] = H[k];
}

__global__ __launch_bounds__(256) void hm_score_kernel(HmBatch b, int max_iters, int it0, int it1)
{
    svo_chain_priority();
    const HmJob &job = b.j[blockIdx.y];
    const int n = job.n;
    if (n <= MP)
        return;
    const int lim = hm_phase_limit(job, max_iters, it0, it1);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float *__restrict__ p1 = job.p1, *__restrict__ p2 = job.p2;
    for (int it = it0 + (int)blockIdx.x * 4 + wave; it < lim; it += (int)gridDim.x * 4) {
        if (job.nmodels[it] <= 0)
            continue;  // wave-uniform
        float Hf[8];
#pragma unroll
        for (int k = 0; k < 8; k++)
            Hf[k] = (float)job.Hm[(size_t)it * 8 + k];
        int cnt = 0;
        for (int i = lane; i < n; i += 64) {
            const float2 u = hm_pair(p1, i), w = hm_pair(p2, i);
            cnt += hm_error(Hf, u.x, u.y, w.x, w.y) <= job.thr ? 1 : 0;
        }
        cnt = wave_sum_dpp(cnt);
        if (lane == 0)
            job.counts[it] = cnt;
    }
}

__global__ void hm_replay_kernel(HmBatch b, double confidence, int max_iters, int it_end, int first)
{
    const HmJob &job = b.j[blockIdx.x];
    if (threadIdx.x != 0)
        return;
    if (job.n <= MP) {  // no loop: fewer than four pairs (no model) or exactly four (the solver once)
        RansacState r;
        r.niters = 0, r.next_iter = 0, r.best_iter = -1, r.best_model = 0, r.best_count = 0, r.done = 1, r.iters_run = 0;
        r.pad = 0;
        *job.st = r;
        return;
    }
    *job.st = ransac_replay<1>(job.st, first, it_end < max_iters ? it_end : max_iters, max_iters, job.n, confidence, job.nmodels,
                               job.counts, MP);
}

constexpr int tri8(int j, int k) { return j * 8 - j * (j - 1) / 2 + (k - j); }  // j <= k, the upper triangle of 8 x 8

// one pair's share of J^T J (36, upper triangle by rows), J^T r (8) and the cost, at h (h8 = 1)
__device__ __forceinline__ void lm_accumulate(const double (&h)[8], double X, double Y, double x, double y, double (&acc)[45])
{
    double ww = h[6] * X + h[7] * Y + 1.;
    ww = fabs(ww) > DBL_EPSILON ? 1. / ww : 0.;
    const double xi = (h[0] * X + h[1] * Y + h[2]) * ww, yi = (h[3] * X + h[4] * Y + h[5]) * ww;
    const double rx = xi - x, ry = yi - y;
    const double J0[8] = {X * ww, Y * ww, ww, 0., 0., 0., -X * ww * xi, -Y * ww * xi};
    const double J1[8] = {0., 0., 0., X * ww, Y * ww, ww, -X * ww * yi, -Y * ww * yi};
#pragma unroll
    for (int j = 0; j < 8; j++) {
#pragma unroll
        for (int k = j; k < 8; k++)
            acc[tri8(j, k)] += J0[j] * J0[k] + J1[j] * J1[k];
        acc[36 + j] += J0[j] * rx + J1[j] * ry;
    }
    acc[44] += rx * rx + ry * ry;
}

// (A + lambda diag A) d = -g by Cholesky (A: acc[0 .. 35], g: acc[36 .. 43]); false: not positive definite or not finite
__device__ bool lm_step(const double (&acc)[45], double lambda, double (&d)[8])
{
    double L[8][8];
#pragma unroll
    for (int j = 0; j < 8; j++)
#pragma unroll
        for (int i = j; i < 8; i++) {
            double sum = i == j ? acc[tri8(j, j)] + lambda * acc[tri8(j, j)] : acc[tri8(j, i)];
#pragma unroll
            for (int k = 0; k < j; k++)
                sum -= L[i][k] * L[j][k];
            if (i == j) {
                if (!(sum > 0))
                    return false;
                L[j][j] = sqrt(sum);
            } else {
                L[i][j] = sum / L[j][j];
            }
        }
    double yv[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        double sum = -acc[36 + i];
#pragma unroll
        for (int k = 0; k < i; k++)
            sum -= L[i][k] * yv[k];
        yv[i] = sum / L[i][i];
    }
    bool fin = true;
#pragma unroll
    for (int i = 7; i >= 0; i--) {
        double sum = yv[i];
#pragma unroll
        for (int k = i + 1; k < 8; k++)
            sum -= L[k][i] * d[k];
        d[i] = sum / L[i][i];
        fin = fin && isfinite(d[i]);
    }
    return fin;
}

// hm_plan::jacobi_sym<9> by one wave on matrices in LDS: lane k takes row / column k of every rotation, the same operations
__device__ void jacobi9_wave(double (*A)[9], double (*V)[9], int lane)
{
    if (lane < 9)
        for (int j = 0; j < 9; j++)
            V[lane][j] = lane == j ? 1. : 0.;
    wave_lds_fence();
    for (int sweep = 0; sweep < hm_plan::kJacobiSweeps; sweep++) {
        bool rotated = false;
        for (int p = 0; p < 8; p++)
            for (int q = p + 1; q < 9; q++) {
                double c = 1., s = 0.;
                const bool rot = hm_plan::jacobi_angle(A[p][p], A[q][q], A[p][q], c, s);  // wave-uniform
                wave_lds_fence();
                if (!rot)
                    continue;
                rotated = true;
                if (lane < 9) {
                    const double ap = A[lane][p], aq = A[lane][q];
                    A[lane][p] = c * ap - s * aq;
                    A[lane][q] = s * ap + c * aq;
                }
                wave_lds_fence();
                if (lane < 9) {
                    const double ap = A[p][lane], aq = A[q][lane];
                    A[p][lane] = c * ap - s * aq;
                    A[q][lane] = s * ap + c * aq;
                    const double vp = V[lane][p], vq = V[lane][q];
                    V[lane][p] = c * vp - s * vq;
                    V[lane][q] = s * vp + c * vq;
                }
                wave_lds_fence();
            }
        if (!rotated)
            break;
    }
}

// mask, refit, polish and outputs of one problem (the file header)
__global__ __launch_bounds__(256) void hm_finish_kernel(HmBatch b)
{
    const HmJob &job = b.j[blockIdx.x];
    const int n = job.n, tid = threadIdx.x;
    __shared__ double s_red[4 * 45];
    __shared__ double sA[9][9], sV[9][9];
    const RansacState s = *job.st;
    bool have = false;
    const double *Hm = job.Hm;
    if (n == MP) {
        have = job.nmodels[0] > 0;
    } else if (n > MP && s.best_iter >= 0 && s.best_count > 0) {
        have = true;
        Hm = job.Hm + (size_t)s.best_iter * 8;
    }
    double H[9];
#pragma unroll
    for (int k = 0; k < 8; k++)
        H[k] = have ? Hm[k] : 0.;
    H[8] = have ? 1. : 0.;
    int count = have && n == MP ? MP : 0;
    if (!have || n == MP) {
        for (int i = tid; i < n; i += 256)
            job.mask[i] = have ? 1 : 0;
    } else {
        const float *p1 = job.p1, *p2 = job.p2;
        float Hf[8];
#pragma unroll
        for (int k = 0; k < 8; k++)
            Hf[k] = (float)H[k];
        // ---- the loop's mask; the inliers' number and means ----
        double v5[5] = {0., 0., 0., 0., 0.};
        for (int i = tid; i < n; i += 256) {
            const float2 u = hm_pair(p1, i), w = hm_pair(p2, i);
            const bool in = hm_error(Hf, u.x, u.y, w.x, w.y) <= job.thr;
            job.mask[i] = in ? 1 : 0;
            if (in) {
                v5[0] += 1.;
                v5[1] += (double)u.x, v5[2] += (double)u.y, v5[3] += (double)w.x, v5[4] += (double)w.y;
            }
        }
        block_sum<5>(v5, s_red);
        const double cnt = v5[0];
        count = (int)cnt;
        const double c1[2] = {v5[1] / cnt, v5[2] / cnt}, c2[2] = {v5[3] / cnt, v5[4] / cnt};
        double v4[4] = {0., 0., 0., 0.};
        for (int i = tid; i < n; i += 256)
            if (job.mask[i]) {
                const float2 u = hm_pair(p1, i), w = hm_pair(p2, i);
                v4[0] += fabs((double)u.x - c1[0]), v4[1] += fabs((double)u.y - c1[1]);
                v4[2] += fabs((double)w.x - c2[0]), v4[3] += fabs((double)w.y - c2[1]);
            }
        block_sum<4>(v4, s_red);
        if (v4[0] >= DBL_EPSILON && v4[1] >= DBL_EPSILON && v4[2] >= DBL_EPSILON && v4[3] >= DBL_EPSILON) {
            // ---- the refit: L^T L over the inliers, its smallest eigenvector ----
            const double s1[2] = {cnt / v4[0], cnt / v4[1]}, s2[2] = {cnt / v4[2], cnt / v4[3]};
            double acc[45];
#pragma unroll
            for (int k = 0; k < 45; k++)
                acc[k] = 0.;
            for (int i = tid; i < n; i += 256)
                if (job.mask[i]) {
                    const float2 u = hm_pair(p1, i), w = hm_pair(p2, i);
                    const double X = ((double)u.x - c1[0]) * s1[0], Y = ((double)u.y - c1[1]) * s1[1];
                    const double x = ((double)w.x - c2[0]) * s2[0], y = ((double)w.y - c2[1]) * s2[1];
                    const double Lx[9] = {X, Y, 1., 0., 0., 0., -x * X, -x * Y, -x}, Ly[9] = {0., 0., 0., X, Y, 1., -y * X, -y * Y, -y};
                    int m = 0;
#pragma unroll
                    for (int j = 0; j < 9; j++)
#pragma unroll
                        for (int k = j; k < 9; k++)
                            acc[m++] += Lx[j] * Lx[k] + Ly[j] * Ly[k];
                }
            block_sum<45>(acc, s_red);
            if (tid == 0) {
                int m = 0;
#pragma unroll
                for (int j = 0; j < 9; j++)
#pragma unroll
                    for (int k = j; k < 9; k++) {
                        sA[j][k] = sA[k][j] = acc[m];
                        m++;
                    }
            }
            __syncthreads();
            if (tid < 64)
                jacobi9_wave(sA, sV, tid);
            __syncthreads();
            int im = 0;
            for (int k = 1; k < 9; k++)
                im = sA[k][k] < sA[im][im] ? k : im;
            double g[9], Hr[9];
#pragma unroll
            for (int k = 0; k < 9; k++)
                g[k] = sV[k][im];
            if (hm_denormalise(g, c1, s1, c2, s2, Hr))
#pragma unroll
                for (int k = 0; k < 9; k++)
                    H[k] = Hr[k];
        }
        // ---- the polish: every thread holds the same sums and takes the same steps ----
        double h[8], acc[45];
#pragma unroll
        for (int k = 0; k < 8; k++)
            h[k] = H[k];
        auto sums = [&](const double (&hh)[8], double (&out)[45]) {
#pragma unroll
            for (int k = 0; k < 45; k++)
                out[k] = 0.;
            for (int i = tid; i < n; i += 256)
                if (job.mask[i]) {
                    const float2 u = hm_pair(p1, i), w = hm_pair(p2, i);
                    lm_accumulate(hh, (double)u.x, (double)u.y, (double)w.x, (double)w.y, out);
                }
            block_sum<45>(out, s_red);
        };
        sums(h, acc);
        double lambda = 1e-3;
        for (int step = 0; step < LM_STEPS; step++) {
            double d[8], ht[8], acct[45];
            if (!lm_step(acc, lambda, d))
                break;
            double dmax = 0., hmax = 1.;
#pragma unroll
            for (int k = 0; k < 8; k++) {
                ht[k] = h[k] + d[k];
                dmax = fmax(dmax, fabs(d[k]));
            }
            sums(ht, acct);
            if (acct[44] < acc[44]) {
#pragma unroll
                for (int k = 0; k < 8; k++)
                    h[k] = ht[k];
#pragma unroll
                for (int k = 0; k < 45; k++)
                    acc[k] = acct[k];
                lambda *= 0.1;
            } else {
                lambda *= 10.;
            }
#pragma unroll
            for (int k = 0; k < 8; k++)
                hmax = fmax(hmax, fabs(h[k]));
            if (dmax <= 1e-12 * hmax)
                break;
        }
#pragma unroll
        for (int k = 0; k < 8; k++)
            H[k] = h[k];
    }
    if (tid == 0) {
        if (job.H_out)
#pragma unroll
            for (int k = 0; k < 9; k++)
                job.H_out[k] = H[k];
        if (job.count_out)
            *job.count_out = count;
        if (job.iters_out)
            *job.iters_out = n > MP ? s.iters_run : 0;
    }
}

__global__ __launch_bounds__(64) void hm_4pt_kernel(const double *x1, const double *x2, int nsamples, double *H_out, int *ok)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nsamples)
        return;
    double a[4][2], c[4][2], H[9];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        a[k][0] = x1[(size_t)s * 8 + 2 * k], a[k][1] = x1[(size_t)s * 8 + 2 * k + 1];
        c[k][0] = x2[(size_t)s * 8 + 2 * k], c[k][1] = x2[(size_t)s * 8 + 2 * k + 1];
    }
    const bool good = hm_solve4(a, c, H);
#pragma unroll
    for (int k = 0; k < 9; k++)
        H_out[(size_t)s * 9 + k] = good ? H[k] : 0.;
    ok[s] = good ? 1 : 0;
}

// ---- the planar pose: the candidates of decomposeHomographyMat, scored as recoverPose scores its four ------------------
struct HpJob {
    const float *p1, *p2;
    int n;
    double K[4];
    const double *H;
    uint8_t *mask;   // in / out, or null
    uint8_t *good4;  // workspace: 4 x n candidate masks
    int *cnt4;       // workspace: 4 counts (zeroed)
    double *R, *t, *nrm;
    int *good_out;   // 4, or null
};
struct HpBatch {
    HpJob j[SVO_LK_MAX_JOBS];
};
static_assert(sizeof(HpBatch) + 64 <= 4096, "kernel arguments are limited to 4 KB");

// t at unit norm (zero stays zero)
__device__ __forceinline__ void hp_unit(const double *t, double *u)
{
    const double nn = sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
    for (int k = 0; k < 3; k++)
        u[k] = nn > 0 ? t[k] / nn : 0.;
}

// a wave per candidate, a workgroup per 64 points; counts by integer atomics (exact, order-free), as rp_count_kernel
__global__ __launch_bounds__(256) void hp_count_kernel(HpBatch b, double dist)
{
    const HpJob &job = b.j[blockIdx.y];
    if ((int)blockIdx.x * 64 >= job.n)
        return;
    __shared__ double sR[36], sT[12], sN[12];
    __shared__ int s_nsol;
    if (threadIdx.x == 0)
        s_nsol = hm_plan::decompose(job.H, job.K, sR, sT, sN);
    __syncthreads();
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    double P[12], tu[3];
    hp_unit(sT + 3 * w, tu);
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++)
            P[4 * r + c] = sR[9 * w + 3 * r + c];
        P[4 * r + 3] = tu[r];
    }
    const int i = blockIdx.x * 64 + lane;
    bool g = false;
    if (i < job.n) {
        const double x1 = ((double)job.p1[2 * i] - job.K[2]) / job.K[0], y1 = ((double)job.p1[2 * i + 1] - job.K[3]) / job.K[1];
        const double x2 = ((double)job.p2[2 * i] - job.K[2]) / job.K[0], y2 = ((double)job.p2[2 * i + 1] - job.K[3]) / job.K[1];
        g = w < s_nsol && rp_point_good(P, x1, y1, x2, y2, dist) && (!job.mask || job.mask[i] != 0);
        job.good4[(size_t)w * job.n + i] = g ? 1 : 0;
    }
    const int c = __popcll(__ballot(g));
    if (lane == 0 && c)
        atomicAdd(job.cnt4 + w, c);
}

__global__ __launch_bounds__(256) void hp_pick_kernel(HpBatch b)
{
    const HpJob &job = b.j[blockIdx.y];
    __shared__ double sR[36], sT[12], sN[12];
    __shared__ int s_nsol;
    if (threadIdx.x == 0)
        s_nsol = hm_plan::decompose(job.H, job.K, sR, sT, sN);
    __syncthreads();
    const int nsol = s_nsol;
    int pick = 0;
    for (int k = 1; k < nsol; k++)
        pick = job.cnt4[k] > job.cnt4[pick] ? k : pick;  // the first candidate with the largest count
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (job.mask && i < job.n)
        job.mask[i] = nsol > 0 ? job.good4[(size_t)pick * job.n + i] : 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        double tu[3];
        hp_unit(sT + 3 * pick, tu);
        for (int k = 0; k < 9; k++)
            job.R[k] = sR[9 * pick + k];
        for (int k = 0; k < 3; k++) {
            job.t[k] = tu[k];
            job.nrm[k] = sN[3 * pick + k];
        }
        if (job.good_out)
            for (int k = 0; k < 4; k++)
                job.good_out[k] = job.cnt4[k];
    }
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// the problems' offsets (host memory): SVO_ERR_ARG when malformed, else the end of the last problem
int check_offsets(const int *offsets, int nprob, int *total)
{
    SVO_CHECK_ARG(offsets && nprob >= 1 && nprob <= SVO_LK_MAX_JOBS);
    SVO_CHECK_ARG(offsets[0] >= 0);
    for (int k = 0; k < nprob; k++)
        SVO_CHECK_ARG(offsets[k + 1] >= offsets[k]);
    *total = offsets[nprob];
    return SVO_OK;
}

}  // namespace

extern "C" int svo_decompose_homography(const double *H9, const double *K4, double *R, double *t, double *n, int *nsol)
{
    SVO_CHECK_ARG(H9 && K4 && R && t && n && nsol);
    for (int k = 0; k < 9; k++)
        SVO_CHECK_ARG(std::isfinite(H9[k]));
    SVO_CHECK_ARG(K4[0] != 0 && K4[1] != 0 && std::isfinite(K4[0]) && std::isfinite(K4[1]) && std::isfinite(K4[2]) &&
                  std::isfinite(K4[3]));
    *nsol = hm_plan::decompose(H9, K4, R, t, n);
    return SVO_OK;
}

extern "C" int svo_homography_4pt(svo_ctx *ctx, const double *x1, const double *x2, int nsamples, double *H_out, int *ok, int mem)
{
    SVO_CHECK_ARG(ctx && nsamples >= 0 && (mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE));
    if (nsamples == 0)
        return SVO_OK;
    SVO_CHECK_ARG(x1 && x2 && H_out && ok);
    const size_t in_b = (size_t)nsamples * MP * 2 * sizeof(double), h_b = (size_t)nsamples * 9 * sizeof(double);
    const size_t n_b = (size_t)nsamples * sizeof(int);
    const dim3 grid((nsamples + 63) / 64);
    ScopedKernelTime tm(ctx, SVO_K_FRANSAC);
    if (mem == SVO_MEM_DEVICE) {
        hipLaunchKernelGGL(hm_4pt_kernel, grid, dim3(64), 0, ctx->stream, x1, x2, nsamples, H_out, ok);
        SVO_HIP(hipGetLastError());
        return SVO_OK;
    }
    int rc;
    if ((rc = ctx->s_a.ensure(in_b)) || (rc = ctx->s_b.ensure(in_b)) || (rc = ctx->s_c.ensure(h_b)) || (rc = ctx->s_d.ensure(n_b)))
        return rc;
    SVO_HIP(hipMemcpyAsync(ctx->s_a.p, x1, in_b, hipMemcpyHostToDevice, ctx->stream));
    SVO_HIP(hipMemcpyAsync(ctx->s_b.p, x2, in_b, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(hm_4pt_kernel, grid, dim3(64), 0, ctx->stream, ctx->s_a.as<double>(), ctx->s_b.as<double>(), nsamples,
                       ctx->s_c.as<double>(), ctx->s_d.as<int>());
    SVO_HIP(hipGetLastError());
    SVO_HIP(hipMemcpyAsync(H_out, ctx->s_c.p, h_b, hipMemcpyDeviceToHost, ctx->stream));
    SVO_HIP(hipMemcpyAsync(ok, ctx->s_d.p, n_b, hipMemcpyDeviceToHost, ctx->stream));
    SVO_HIP(hipStreamSynchronize(ctx->stream));
    return SVO_OK;
}

extern "C" int svo_find_homography(svo_ctx *ctx, const float *p1, const float *p2, const int *offsets, int nprob, double threshold,
                                   double confidence, int max_iters, uint64_t seed, uint8_t *mask, double *H_out,
                                   int *inlier_count, int *iters_run, int mem)
{
    SVO_CHECK_ARG(ctx && (mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE));
    int total = 0, rc;
    if ((rc = check_offsets(offsets, nprob, &total)))
        return rc;
    SVO_CHECK_ARG(threshold > 0 && std::isfinite(threshold) && confidence > 0 && confidence < 1);
    SVO_CHECK_ARG(max_iters >= 1 && max_iters <= MAX_ITERS);
    SVO_CHECK_ARG(total == 0 || (p1 && p2 && mask));
    const int base = offsets[0];
    // workspace per problem: the models, then the state / model counts / inlier counts
    const size_t hm_b = align256((size_t)max_iters * 8 * sizeof(double));
    const size_t ct_b = align256((size_t)max_iters * 2 * sizeof(int) + sizeof(RansacState));
    const size_t ws = (size_t)nprob * (hm_b + ct_b);
    // host mode: the staged inputs and outputs behind the workspace
    const size_t pin_b = align256((size_t)(total + 1) * 2 * sizeof(float)), mask_b = align256((size_t)total + 1);
    const size_t out_b = align256((size_t)nprob * (9 * sizeof(double) + 2 * sizeof(int)));
    const size_t stage = mem == SVO_MEM_HOST ? 2 * pin_b + mask_b + out_b : 0;
    if ((rc = ctx->ess.ensure(ws + stage)))
        return rc;
    char *w = ctx->ess.as<char>();
    const float *d1 = p1, *d2 = p2;
    uint8_t *dmask = mask;
    double *dH = H_out;
    int *dcnt = inlier_count, *dit = iters_run;
    if (mem == SVO_MEM_HOST) {
        char *stg = w + ws;
        float *s1 = reinterpret_cast<float *>(stg), *s2 = reinterpret_cast<float *>(stg + pin_b);
        if (total > base) {
            SVO_HIP(hipMemcpyAsync(s1 + 2 * base, p1 + 2 * base, (size_t)(total - base) * 8, hipMemcpyHostToDevice, ctx->stream));
            SVO_HIP(hipMemcpyAsync(s2 + 2 * base, p2 + 2 * base, (size_t)(total - base) * 8, hipMemcpyHostToDevice, ctx->stream));
        }
        d1 = s1, d2 = s2;
        dmask = reinterpret_cast<uint8_t *>(stg + 2 * pin_b);
        dH = reinterpret_cast<double *>(stg + 2 * pin_b + mask_b);
        dcnt = reinterpret_cast<int *>(dH + (size_t)nprob * 9);
        dit = dcnt + nprob;
    }
    HmBatch b;
    int nmax = 0;
    for (int k = 0; k < nprob; k++) {
        HmJob &j = b.j[k];
        const int o = offsets[k], n = offsets[k + 1] - offsets[k];
        j.p1 = d1 ? d1 + 2 * (size_t)o : nullptr;
        j.p2 = d2 ? d2 + 2 * (size_t)o : nullptr;
        j.n = n;
        j.thr = (float)(threshold * threshold);
        char *pw = w + (size_t)k * (hm_b + ct_b);
        j.Hm = reinterpret_cast<double *>(pw);
        j.st = reinterpret_cast<RansacState *>(pw + hm_b);
        j.nmodels = reinterpret_cast<int *>(j.st + 1);
        j.counts = j.nmodels + max_iters;
        j.mask = dmask ? dmask + o : nullptr;
        j.H_out = dH ? dH + (size_t)k * 9 : nullptr;
        j.count_out = dcnt ? dcnt + k : nullptr;
        j.iters_out = dit ? dit + k : nullptr;
        nmax = n > nmax ? n : nmax;
    }
    for (int k = nprob; k < SVO_LK_MAX_JOBS; k++)
        b.j[k] = b.j[0];
    {
        ScopedKernelTime tm(ctx, SVO_K_FRANSAC);
        const int bounds[3] = {0, 64, 256};
        for (int ph = 0; ph < 3; ph++) {
            const int it0 = bounds[ph];
            const int it1 = ph == 2 ? max_iters : (bounds[ph + 1] < max_iters ? bounds[ph + 1] : max_iters);
            if (it0 >= it1)
                break;
            const int its = it1 - it0;
            hipLaunchKernelGGL(hm_solve_kernel, dim3((its + 63) / 64, nprob), dim3(64), 0, ctx->stream, b, seed, max_iters, it0, it1);
            if (nmax > MP)
                hipLaunchKernelGGL(hm_score_kernel, dim3((its + 3) / 4 < 1024 ? (its + 3) / 4 : 1024, nprob), dim3(256), 0, ctx->stream, b,
                                   max_iters, it0, it1);
            hipLaunchKernelGGL(hm_replay_kernel, dim3(nprob), dim3(64), 0, ctx->stream, b, confidence, max_iters, it1, ph == 0 ? 1 : 0);
        }
        hipLaunchKernelGGL(hm_finish_kernel, dim3(nprob), dim3(256), 0, ctx->stream, b);
        SVO_HIP(hipGetLastError());
    }
    if (mem == SVO_MEM_DEVICE)
        return SVO_OK;
    if (total > base)
        SVO_HIP(hipMemcpyAsync(mask + base, dmask + base, (size_t)(total - base), hipMemcpyDeviceToHost, ctx->stream));
    if (H_out)
        SVO_HIP(hipMemcpyAsync(H_out, dH, (size_t)nprob * 9 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (inlier_count)
        SVO_HIP(hipMemcpyAsync(inlier_count, dcnt, (size_t)nprob * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    if (iters_run)
        SVO_HIP(hipMemcpyAsync(iters_run, dit, (size_t)nprob * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    SVO_HIP(hipStreamSynchronize(ctx->stream));
    return SVO_OK;
}

extern "C" int svo_homography_pose(svo_ctx *ctx, const double *H9, const float *p1, const float *p2, const int *offsets, int nprob,
                                   const double *K4, double distance_thresh, uint8_t *mask_inout, double *R9, double *t3,
                                   double *n3, int *good4, int mem)
{
    SVO_CHECK_ARG(ctx && (mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE));
    int total = 0, rc;
    if ((rc = check_offsets(offsets, nprob, &total)))
        return rc;
    SVO_CHECK_ARG(K4);
    for (int k = 0; k < nprob; k++)
        SVO_CHECK_ARG(K4[4 * k] != 0 && K4[4 * k + 1] != 0 && std::isfinite(K4[4 * k]) && std::isfinite(K4[4 * k + 1]) &&
                      std::isfinite(K4[4 * k + 2]) && std::isfinite(K4[4 * k + 3]));
    SVO_CHECK_ARG(H9 && R9 && t3 && n3 && distance_thresh > 0);
    SVO_CHECK_ARG(total == 0 || (p1 && p2));
    const int base = offsets[0];
    const size_t g_b = align256((size_t)4 * (total + 1)), c_b = align256((size_t)nprob * 4 * sizeof(int));
    const size_t pin_b = align256((size_t)(total + 1) * 2 * sizeof(float)), mask_b = align256((size_t)total + 1);
    const size_t ho_b = align256((size_t)nprob * (9 + 9 + 3 + 3) * sizeof(double) + (size_t)nprob * 4 * sizeof(int));
    const size_t stage = mem == SVO_MEM_HOST ? 2 * pin_b + mask_b + ho_b : 0;
    if ((rc = ctx->ess.ensure(g_b + c_b + stage)))
        return rc;
    char *w = ctx->ess.as<char>();
    uint8_t *cand = reinterpret_cast<uint8_t *>(w);
    int *cnt = reinterpret_cast<int *>(w + g_b);
    const float *d1 = p1, *d2 = p2;
    const double *dH = H9;
    uint8_t *dmask = mask_inout;
    double *dR = R9, *dt = t3, *dn = n3;
    int *dgood = good4;
    if (mem == SVO_MEM_HOST) {
        char *stg = w + g_b + c_b;
        float *s1 = reinterpret_cast<float *>(stg), *s2 = reinterpret_cast<float *>(stg + pin_b);
        if (total > base) {
            SVO_HIP(hipMemcpyAsync(s1 + 2 * base, p1 + 2 * base, (size_t)(total - base) * 8, hipMemcpyHostToDevice, ctx->stream));
            SVO_HIP(hipMemcpyAsync(s2 + 2 * base, p2 + 2 * base, (size_t)(total - base) * 8, hipMemcpyHostToDevice, ctx->stream));
        }
        d1 = s1, d2 = s2;
        dmask = mask_inout ? reinterpret_cast<uint8_t *>(stg + 2 * pin_b) : nullptr;
        if (mask_inout && total > base)
            SVO_HIP(hipMemcpyAsync(dmask + base, mask_inout + base, (size_t)(total - base), hipMemcpyHostToDevice, ctx->stream));
        double *ho = reinterpret_cast<double *>(stg + 2 * pin_b + mask_b);
        SVO_HIP(hipMemcpyAsync(ho, H9, (size_t)nprob * 9 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        dH = ho;
        dR = ho + (size_t)nprob * 9;
        dt = dR + (size_t)nprob * 9;
        dn = dt + (size_t)nprob * 3;
        dgood = reinterpret_cast<int *>(dn + (size_t)nprob * 3);
    }
    SVO_HIP(hipMemsetAsync(cnt, 0, (size_t)nprob * 4 * sizeof(int), ctx->stream));
    HpBatch b;
    int nmax = 0;
    for (int k = 0; k < nprob; k++) {
        HpJob &j = b.j[k];
        const int o = offsets[k], n = offsets[k + 1] - offsets[k];
        j.p1 = d1 ? d1 + 2 * (size_t)o : nullptr;
        j.p2 = d2 ? d2 + 2 * (size_t)o : nullptr;
        j.n = n;
        for (int m = 0; m < 4; m++)
            j.K[m] = K4[4 * k + m];
        j.H = dH + 9 * (size_t)k;
        j.mask = dmask ? dmask + o : nullptr;
        j.good4 = cand + 4 * (size_t)o;
        j.cnt4 = cnt + 4 * k;
        j.R = dR + 9 * (size_t)k;
        j.t = dt + 3 * (size_t)k;
        j.nrm = dn + 3 * (size_t)k;
        j.good_out = dgood ? dgood + 4 * k : nullptr;
        nmax = n > nmax ? n : nmax;
    }
    for (int k = nprob; k < SVO_LK_MAX_JOBS; k++)
        b.j[k] = b.j[0];
    {
        ScopedKernelTime tm(ctx, SVO_K_TRIANGULATE);
        if (nmax > 0)
            hipLaunchKernelGGL(hp_count_kernel, dim3((nmax + 63) / 64, nprob), dim3(256), 0, ctx->stream, b, distance_thresh);
        hipLaunchKernelGGL(hp_pick_kernel, dim3(nmax > 0 ? (nmax + 255) / 256 : 1, nprob), dim3(256), 0, ctx->stream, b);
        SVO_HIP(hipGetLastError());
    }
    if (mem == SVO_MEM_DEVICE)
        return SVO_OK;
    if (mask_inout && total > base)
        SVO_HIP(hipMemcpyAsync(mask_inout + base, dmask + base, (size_t)(total - base), hipMemcpyDeviceToHost, ctx->stream));
    SVO_HIP(hipMemcpyAsync(R9, dR, (size_t)nprob * 9 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    SVO_HIP(hipMemcpyAsync(t3, dt, (size_t)nprob * 3 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    SVO_HIP(hipMemcpyAsync(n3, dn, (size_t)nprob * 3 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (good4)
        SVO_HIP(hipMemcpyAsync(good4, dgood, (size_t)nprob * 4 * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    SVO_HIP(hipStreamSynchronize(ctx->stream));
    return SVO_OK;
}
