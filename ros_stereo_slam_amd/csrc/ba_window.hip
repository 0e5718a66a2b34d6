// ba_window.hip -- windowed bundle adjustment: up to 16 free (and 16 more held) poses, N free marginalised points, mono and
// stereo observations stored CSR by point (gfx950).  OURS in scope -- upstream only names it as future work -- and g2o's in
// arithmetic: OptimizationAlgorithmLevenberg over BlockSolver<6,3>, EdgeSE3ProjectXYZ / EdgeStereoSE3ProjectXYZ with identity
// information and RobustKernelHuber as robustify applies it, the control flow of ba.hip.
//
// Mapping.  The Levenberg-Marquardt state (lambda, nu, the accepted chi2) lives on the HOST, which reads one 64-byte record per
// trial and applies ba_window_plan::lm_trial; a trial is five launches on the context's stream:
//   1. bw_schur_kernel    grid over points, ONE WAVEFRONT per workgroup owning CHUNK = 32 consecutive points.  The wave walks its
//                         points one after the other.  Lane l linearises observation l of the point (a run holds at most 32);
//                         the 3x3 block Hll and bl are the sum of the lanes' terms IN CSR ORDER (through LDS, every lane adds
//                         them up redundantly); every free observation's coupling block Hpl (6x3) and Hpl V^-1 go to LDS, then
//                         36 lanes add Hpl_a V^-1 Hpl_b^T into block (a, b >= a) of the workgroup's packed upper triangle in
//                         LDS and 6 lanes Hpl_a V^-1 bl into its right-hand side; Hpp / bp of the free poses likewise.  A point
//                         is seen at most once by a pose, so within a point no two lanes meet at an address; points follow in
//                         index order (LDS operations of one wave execute in order).  The workgroup writes its slab.
//   2. bw_reduce_kernel   one thread per slab entry adds the slabs IN SLAB ORDER (chi2 too; max |diag Hll| by fmax).
//   3. bw_solve_kernel    one workgroup: S = Hpp + lambda I - sum, right-looking Cholesky on the packed lower triangle in LDS
//                         (every entry takes its subtractions in ascending pivot order), the two substitutions, SE3Quat::exp on
//                         every free pose -> trial poses, dp, the poses' share of the gain-ratio scale.  A pivot that is not
//                         positive rejects the trial.
//   4. bw_backsub_kernel  one thread per point: Hll, bl and sum_j Hpl_j^T dp_j over its run in CSR order, dl = V^-1 (bl - ...),
//                         the trial point, the trial residuals under the trial poses; dl (lambda dl + bl) and rho(e^2) are
//                         summed per workgroup by svo::block_sum (butterfly per wave, then ((w0 + w1) + w2) + w3) into a slab.
//   5. bw_record_kernel   one thread adds those slabs in slab order and writes the record.
// An accepted trial swaps the estimate and trial buffers on the host (no copy).  No atomics, no grid-wide barrier: every sum
// above has one order, so two runs give the same bits.
// Bound: 1 and 4 by f64 VALU latency (few waves, ~1 kflop per observation, recomputed instead of stored: 288 B per observation
// per pass otherwise); 2 by the slab traffic (slabs x stride x 8 B, L2-resident); 3 by LDS latency and barriers of one workgroup
// (about 3 x dim barriers); the trial as a whole by five launches and one host wait.
#include "ba_window_plan.hip.h"
#include "se3_solve.hip.h"
#include "svo_internal.h"
#include "wave_ops.hip.h"

namespace {

namespace plan = ba_window_plan;

struct BwCam {
    double fx, fy, cx, cy, bf, huber_mono, huber_stereo;
};

struct BwLin {
    double e[3], A[9], B[18];  // residuals, d e / d point (3 x 3), d e / d pose (3 x 6, [omega; upsilon]); row 2 zero when mono
    double w, rho;             // g2o's rho[1] and rho[0]
};

// residuals of one observation; xc: the point in the camera
__device__ __forceinline__ bool bw_error(const double *P, const double *X, float zu, float zv, float zr, const BwCam &c,
                                         double *e, double *xc)
{
    const double x = P[0] * X[0] + P[1] * X[1] + P[2] * X[2] + P[9];
    const double y = P[3] * X[0] + P[4] * X[1] + P[5] * X[2] + P[10];
    const double w = P[6] * X[0] + P[7] * X[1] + P[8] * X[2] + P[11];
    const bool stereo = !isnan(zr);
    e[0] = (double)zu - (x / w * c.fx + c.cx);
    e[1] = (double)zv - (y / w * c.fy + c.cy);
    e[2] = stereo ? (double)zr - (x / w * c.fx + c.cx - c.bf / w) : 0.;
    xc[0] = x;
    xc[1] = y;
    xc[2] = w;
    return stereo;
}

// RobustKernelHuber::robustify on e2 = e^T e; delta == 0: no kernel (rho = e2, weight 1: the products below are then exact)
__device__ __forceinline__ void bw_robust(double e2, double delta, double &rho, double &w)
{
    if (delta > 0. && e2 > delta * delta) {
        const double s = sqrt(e2);
        rho = 2. * s * delta - delta * delta;
        w = delta / s;
    } else {
        rho = e2;
        w = 1.;
    }
}

__device__ __forceinline__ double bw_chi(const double *P, const double *X, float zu, float zv, float zr, const BwCam &c, double *e2)
{
    double e[3], xc[3], rho, w;
    const bool stereo = bw_error(P, X, zu, zv, zr, c, e, xc);
    const double q = e[0] * e[0] + e[1] * e[1] + e[2] * e[2];
    if (e2)
        *e2 = q;
    bw_robust(q, stereo ? c.huber_stereo : c.huber_mono, rho, w);
    return rho;
}

// EdgeSE3ProjectXYZ / EdgeStereoSE3ProjectXYZ::linearizeOplus (g2o types_six_dof_expmap)
__device__ __forceinline__ void bw_linearize(const double *P, const double *X, float zu, float zv, float zr, const BwCam &c, BwLin &L)
{
    double xc[3];
    const bool stereo = bw_error(P, X, zu, zv, zr, c, L.e, xc);
    bw_robust(L.e[0] * L.e[0] + L.e[1] * L.e[1] + L.e[2] * L.e[2], stereo ? c.huber_stereo : c.huber_mono, L.rho, L.w);
    const double x = xc[0], y = xc[1], z = xc[2], z2 = z * z;
    const double bfz2 = stereo ? c.bf / z2 : 0.;
    // NOT shared with ba_linearize's A: the two round differently, each pinned to its own checker -- do not unify
#pragma unroll
    for (int k = 0; k < 3; k++) {
        L.A[k] = -c.fx * P[k] / z + c.fx * x * P[6 + k] / z2;
        L.A[3 + k] = -c.fy * P[3 + k] / z + c.fy * y * P[6 + k] / z2;
        L.A[6 + k] = stereo ? L.A[k] - bfz2 * P[6 + k] : 0.;
    }
    svo::project_pose_jacobian(x, y, z, c.fx, c.fy, L.B);
    L.B[12] = stereo ? L.B[0] - bfz2 * y : 0.;
    L.B[13] = stereo ? L.B[1] + bfz2 * x : 0.;
    L.B[14] = stereo ? L.B[2] : 0.;
    L.B[15] = stereo ? L.B[3] : 0.;
    L.B[16] = 0.;
    L.B[17] = stereo ? L.B[5] - bfz2 : 0.;
}

// one observation's terms of its point's block: w A^T A (packed 00 01 02 11 12 22) and -w A^T e
__device__ __forceinline__ void bw_point_terms(const BwLin &L, double *H, double *b)
{
    const double *A = L.A;
    H[0] = L.w * (A[0] * A[0] + A[3] * A[3] + A[6] * A[6]);
    H[1] = L.w * (A[0] * A[1] + A[3] * A[4] + A[6] * A[7]);
    H[2] = L.w * (A[0] * A[2] + A[3] * A[5] + A[6] * A[8]);
    H[3] = L.w * (A[1] * A[1] + A[4] * A[4] + A[7] * A[7]);
    H[4] = L.w * (A[1] * A[2] + A[4] * A[5] + A[7] * A[8]);
    H[5] = L.w * (A[2] * A[2] + A[5] * A[5] + A[8] * A[8]);
#pragma unroll
    for (int k = 0; k < 3; k++)
        b[k] = -(L.w * (A[k] * L.e[0] + A[3 + k] * L.e[1] + A[6 + k] * L.e[2]));
}

// the coupling block Hpl = w B^T A, 6 x 3 row-major
__device__ __forceinline__ void bw_coupling(const BwLin &L, double *Hpl)
{
#pragma unroll
    for (int r = 0; r < 6; r++)
#pragma unroll
        for (int k = 0; k < 3; k++)
            Hpl[3 * r + k] = L.w * (L.B[r] * L.A[k] + L.B[6 + r] * L.A[3 + k] + L.B[12 + r] * L.A[6 + k]);
}

// device -> host record of one trial (and of the first look at the problem)
struct BwRecord {
    double solved, temp_chi, scale, chi, max_diag, pad[3];
};

struct BwProblem {
    BwCam cam;
    int n_points, n_poses, n_free;
    plan::SlabLayout lay;
    const float *pts3d;
    const int *obs_start, *obs_pose;
    const float *obs_uvr;
    signed char free_index[plan::MAX_POSES];
    signed char free_list[plan::MAX_FREE];
};

__global__ __launch_bounds__(256) void bw_init_points_kernel(const float *__restrict__ pts3d, int n3, double *__restrict__ X)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n3)
        X[i] = (double)pts3d[i];
}

constexpr int BW_PT = 10;  // doubles a lane leaves for its point: 6 of Hll, 3 of bl, rho

// SCHUR == false: the first look (chi2, Hpp, bp, max |diag Hll|; lambda is not read)
template <bool SCHUR>
__global__ __launch_bounds__(64) void bw_schur_kernel(BwProblem q, const double *__restrict__ poses, const double *__restrict__ X,
                                                      double lambda, double *__restrict__ slabs)
{
    extern __shared__ double s_dyn[];
    const int lane = threadIdx.x, stride = q.lay.stride, dim = q.lay.dim;
    double *s_slab = s_dyn;                         // [stride]
    double *s_pt = s_slab + stride;                 // [32][BW_PT]
    double *s_W = s_pt + plan::MAX_POSES * BW_PT;   // [32][18] Hpl
    double *s_Y = s_W + plan::MAX_POSES * 18;       // [32][18] Hpl V^-1
    int *s_f = reinterpret_cast<int *>(s_Y + plan::MAX_POSES * 18);  // [32] row block of the lane's pose, -1: held
    int *s_fi = s_f + plan::MAX_POSES;                                // [32] pose -> row block
    for (int k = lane; k < stride; k += 64)
        s_slab[k] = 0.;
    if (lane < plan::MAX_POSES)
        s_fi[lane] = lane < q.n_poses ? (int)q.free_index[lane] : -1;
    svo::wave_lds_fence();
    double *s_S = s_slab, *s_sb = s_slab + q.lay.off_sb, *s_hpp = s_slab + q.lay.off_hpp, *s_bp = s_slab + q.lay.off_bp;
    double chi = 0., md = 0.;
    const int p0 = blockIdx.x * plan::CHUNK, p1 = min(p0 + plan::CHUNK, q.n_points);
    const int er = lane / 6, ec = lane - 6 * er;  // the entry of a 6 x 6 block lanes 0..35 own
    for (int p = p0; p < p1; p++) {
        const int o0 = q.obs_start[p], m = q.obs_start[p + 1] - o0;
        if (m == 0)
            continue;
        const bool active = lane < m;
        BwLin L;
        int f = -1;
        if (active) {
            const int o = o0 + lane, j = q.obs_pose[o];
            f = s_fi[j];
            const double Xp[3] = {X[3 * (size_t)p], X[3 * (size_t)p + 1], X[3 * (size_t)p + 2]};
            bw_linearize(poses + 12 * j, Xp, q.obs_uvr[3 * (size_t)o], q.obs_uvr[3 * (size_t)o + 1], q.obs_uvr[3 * (size_t)o + 2],
                         q.cam, L);
            double H[6], b[3];
            bw_point_terms(L, H, b);
#pragma unroll
            for (int k = 0; k < 6; k++)
                s_pt[lane * BW_PT + k] = H[k];
#pragma unroll
            for (int k = 0; k < 3; k++)
                s_pt[lane * BW_PT + 6 + k] = b[k];
            s_pt[lane * BW_PT + 9] = L.rho;
            s_f[lane] = f;
        }
        svo::wave_lds_fence();
        double Hll[6] = {0, 0, 0, 0, 0, 0}, bl[3] = {0, 0, 0};
        for (int l = 0; l < m; l++) {  // CSR order, the same in every lane
#pragma unroll
            for (int k = 0; k < 6; k++)
                Hll[k] += s_pt[l * BW_PT + k];
#pragma unroll
            for (int k = 0; k < 3; k++)
                bl[k] += s_pt[l * BW_PT + 6 + k];
            chi += s_pt[l * BW_PT + 9];
        }
        md = fmax(md, fmax(Hll[0], fmax(Hll[3], Hll[5])));
        double Vi[6] = {0, 0, 0, 0, 0, 0};
        if (SCHUR)
            svo::sym3_inv_damped(Hll, lambda, Vi);
        if (active && f >= 0) {
            if (SCHUR) {
                double Hpl[18], Y[18];
                bw_coupling(L, Hpl);
                svo::sym3_mul_rows6(Hpl, Vi, Y);
#pragma unroll
                for (int k = 0; k < 18; k++) {
                    s_W[lane * 18 + k] = Hpl[k];
                    s_Y[lane * 18 + k] = Y[k];
                }
            }
            // the pose's own block: no other lane of this point holds the same pose
            int k = 0;
#pragma unroll
            for (int r = 0; r < 6; r++)
#pragma unroll
                for (int c = r; c < 6; c++) {
                    s_hpp[21 * f + k] += L.w * (L.B[r] * L.B[c] + L.B[6 + r] * L.B[6 + c] + L.B[12 + r] * L.B[12 + c]);
                    k++;
                }
#pragma unroll
            for (int r = 0; r < 6; r++)
                s_bp[6 * f + r] += -(L.w * (L.B[r] * L.e[0] + L.B[6 + r] * L.e[1] + L.B[12 + r] * L.e[2]));
        }
        svo::wave_lds_fence();
        if (SCHUR) {
            for (int a = 0; a < m; a++) {
                const int fa = s_f[a];
                if (fa < 0)
                    continue;
                const double *Ya = s_Y + a * 18;
                if (lane < 6)
                    s_sb[6 * fa + lane] += Ya[3 * lane] * bl[0] + Ya[3 * lane + 1] * bl[1] + Ya[3 * lane + 2] * bl[2];
                for (int b = 0; b < m; b++) {
                    const int fb = s_f[b];
                    if (fb < fa)
                        continue;
                    if (lane < 36 && (fa != fb || er <= ec)) {
                        const double *Wb = s_W + b * 18;
                        const int row = 6 * fa + er, col = 6 * fb + ec;
                        s_S[row * dim - row * (row - 1) / 2 + (col - row)] +=
                            Ya[3 * er] * Wb[3 * ec] + Ya[3 * er + 1] * Wb[3 * ec + 1] + Ya[3 * er + 2] * Wb[3 * ec + 2];
                    }
                }
            }
        }
        svo::wave_lds_fence();
    }
    if (lane == 0) {
        s_slab[q.lay.off_chi] = chi;
        s_slab[q.lay.off_max] = md;
    }
    svo::wave_lds_fence();
    double *out = slabs + (size_t)blockIdx.x * stride;
    for (int k = lane; k < stride; k += 64)
        out[k] = s_slab[k];
}

// entry k of every slab, in slab order
__global__ __launch_bounds__(256) void bw_reduce_kernel(const double *__restrict__ slabs, int n_slabs, int stride, int off_max,
                                                        double *__restrict__ out)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= stride)
        return;
    double acc = slabs[k];
    if (k == off_max) {
        for (int s = 1; s < n_slabs; s++)
            acc = fmax(acc, slabs[(size_t)s * stride + k]);
    } else {
        for (int s = 1; s < n_slabs; s++)
            acc += slabs[(size_t)s * stride + k];
    }
    out[k] = acc;
}

__device__ __forceinline__ int bw_low(int i, int j) { return i * (i + 1) / 2 + j; }  // packed lower triangle, i >= j

__global__ __launch_bounds__(256) void bw_solve_kernel(BwProblem q, const double *__restrict__ red, double lambda,
                                                       const double *__restrict__ poses, double *__restrict__ trial,
                                                       double *__restrict__ dp_out, BwRecord *rec)
{
    __shared__ double s_L[plan::MAX_DIM * (plan::MAX_DIM + 1) / 2];
    __shared__ double s_b[plan::MAX_DIM];
    const int tid = threadIdx.x, dim = q.lay.dim;
    const double *hpp = red + q.lay.off_hpp, *bp = red + q.lay.off_bp;
    // S = Hpp + lambda I - sum, lower triangle (i >= j) from the packed upper one
    for (int i = tid >> 4; i < dim; i += 16)
        for (int j = tid & 15; j <= i; j += 16) {
            const int fi = i / 6, fj = j / 6;
            double h = 0.;
            if (fi == fj) {
                const int r = j - 6 * fj, c = i - 6 * fi;
                h = hpp[21 * fi + 6 * r - r * (r - 1) / 2 + (c - r)];
            }
            s_L[bw_low(i, j)] = h + (i == j ? lambda : 0.) - red[j * dim - j * (j - 1) / 2 + (i - j)];
        }
    for (int i = tid; i < dim; i += 256)
        s_b[i] = bp[i] - red[q.lay.off_sb + i];
    __syncthreads();
    bool ok = true;
    const int ti = tid >> 4, tj = tid & 15;
    for (int k = 0; k < dim; k++) {
        const double d = s_L[bw_low(k, k)];
        if (!(d > 0)) {  // the same value in every thread
            ok = false;
            break;
        }
        __syncthreads();
        const double s = sqrt(d);
        if (tid == 0)
            s_L[bw_low(k, k)] = s;
        for (int i = k + 1 + tid; i < dim; i += 256)
            s_L[bw_low(i, k)] = s_L[bw_low(i, k)] / s;
        __syncthreads();
        for (int i = k + 1 + ti; i < dim; i += 16) {
            const double lik = s_L[bw_low(i, k)];
            for (int j = k + 1 + tj; j <= i; j += 16)
                s_L[bw_low(i, j)] -= lik * s_L[bw_low(j, k)];
        }
        __syncthreads();
    }
    if (ok) {
        for (int k = 0; k < dim; k++) {  // L y = b
            if (tid == 0)
                s_b[k] = s_b[k] / s_L[bw_low(k, k)];
            __syncthreads();
            const double yk = s_b[k];
            for (int i = k + 1 + tid; i < dim; i += 256)
                s_b[i] -= s_L[bw_low(i, k)] * yk;
            __syncthreads();
        }
        for (int k = dim - 1; k >= 0; k--) {  // L^T x = y
            if (tid == 0)
                s_b[k] = s_b[k] / s_L[bw_low(k, k)];
            __syncthreads();
            const double xk = s_b[k];
            for (int i = tid; i < k; i += 256)
                s_b[i] -= s_L[bw_low(k, i)] * xk;
            __syncthreads();
        }
    }
    // trial poses: the held ones as they are, exp(dp) * pose for the free ones
    for (int k = tid; k < 12 * q.n_poses; k += 256)
        trial[k] = poses[k];
    __syncthreads();
    if (ok && tid < q.n_free) {
        const int j = q.free_list[tid];
        double d[6], P[12], Pn[12];
        for (int k = 0; k < 6; k++)
            d[k] = s_b[6 * tid + k];
        for (int k = 0; k < 12; k++)
            P[k] = poses[12 * j + k];
        svo::se3_exp_mul(d, P, P + 9, Pn, Pn + 9);
        for (int k = 0; k < 12; k++)
            trial[12 * j + k] = Pn[k];
    }
    if (ok)
        for (int i = tid; i < dim; i += 256)
            dp_out[i] = s_b[i];
    if (tid == 0) {
        double sc = 0.;
        if (ok)
            for (int r = 0; r < dim; r++)
                sc += s_b[r] * (lambda * s_b[r] + bp[r]);
        rec->solved = ok ? 1. : 0.;
        rec->scale = sc;  // the poses' share; bw_record_kernel adds the points'
    }
}

__global__ __launch_bounds__(plan::BLOCK) void bw_backsub_kernel(BwProblem q, const double *__restrict__ poses,
                                                                const double *__restrict__ trial, const double *__restrict__ X,
                                                                double *__restrict__ Xn, const double *__restrict__ dp,
                                                                double lambda, const BwRecord *rec, double *__restrict__ slabs)
{
    __shared__ double s_red[4 * 2];
    __shared__ double s_dp[plan::MAX_DIM];
    __shared__ int s_fi[plan::MAX_POSES];
    if (rec->solved == 0.)  // a failed factorisation: the trial is rejected, nothing of it is read
        return;
    const int tid = threadIdx.x, p = blockIdx.x * plan::BLOCK + tid;
    for (int k = tid; k < q.lay.dim; k += plan::BLOCK)
        s_dp[k] = dp[k];
    if (tid < plan::MAX_POSES)
        s_fi[tid] = tid < q.n_poses ? (int)q.free_index[tid] : -1;
    __syncthreads();
    double c2[2] = {0., 0.};
    if (p < q.n_points) {
        const int o0 = q.obs_start[p], o1 = q.obs_start[p + 1];
        const double Xp[3] = {X[3 * (size_t)p], X[3 * (size_t)p + 1], X[3 * (size_t)p + 2]};
        double xn[3] = {Xp[0], Xp[1], Xp[2]};
        if (o1 > o0) {
            double Hll[6] = {0, 0, 0, 0, 0, 0}, bl[3] = {0, 0, 0}, hd[3] = {0, 0, 0};
            for (int o = o0; o < o1; o++) {
                const int j = q.obs_pose[o], f = s_fi[j];
                BwLin L;
                bw_linearize(poses + 12 * j, Xp, q.obs_uvr[3 * (size_t)o], q.obs_uvr[3 * (size_t)o + 1], q.obs_uvr[3 * (size_t)o + 2],
                             q.cam, L);
                double H[6], b[3];
                bw_point_terms(L, H, b);
#pragma unroll
                for (int k = 0; k < 6; k++)
                    Hll[k] += H[k];
#pragma unroll
                for (int k = 0; k < 3; k++)
                    bl[k] += b[k];
                if (f >= 0) {  // Hpl^T dp of this observation
                    double Hpl[18];
                    bw_coupling(L, Hpl);
#pragma unroll
                    for (int k = 0; k < 3; k++) {
                        double s = 0;
#pragma unroll
                        for (int r = 0; r < 6; r++)
                            s += Hpl[3 * r + k] * s_dp[6 * f + r];
                        hd[k] += s;
                    }
                }
            }
            double Vi[6], r3[3], dl[3];
            svo::sym3_inv_damped(Hll, lambda, Vi);
#pragma unroll
            for (int k = 0; k < 3; k++)
                r3[k] = bl[k] - hd[k];
            svo::sym3_mul_vec(Vi, r3, dl);
#pragma unroll
            for (int k = 0; k < 3; k++) {
                xn[k] = Xp[k] + dl[k];
                c2[0] += dl[k] * (lambda * dl[k] + bl[k]);
            }
            for (int o = o0; o < o1; o++)
                c2[1] += bw_chi(trial + 12 * q.obs_pose[o], xn, q.obs_uvr[3 * (size_t)o], q.obs_uvr[3 * (size_t)o + 1],
                                q.obs_uvr[3 * (size_t)o + 2], q.cam, nullptr);
        }
#pragma unroll
        for (int k = 0; k < 3; k++)
            Xn[3 * (size_t)p + k] = xn[k];
    }
    svo::block_sum<2>(c2, s_red);
    if (tid == 0) {
        slabs[2 * blockIdx.x] = c2[0];
        slabs[2 * blockIdx.x + 1] = c2[1];
    }
}

// first == 1: the first look's record from the summed slabs (chi2, max |diag H| over point AND pose blocks);
// else a trial's: its chi2 and gain-ratio scale from the back-substitution's slabs in slab order
__global__ void bw_record_kernel(BwProblem q, int first, const double *__restrict__ red, const double *__restrict__ slabs,
                                 int n_slabs, BwRecord *rec)
{
    if (threadIdx.x != 0 || blockIdx.x != 0)
        return;
    if (first) {
        double md = red[q.lay.off_max];
        for (int f = 0; f < q.n_free; f++)
            for (int r = 0; r < 6; r++)
                md = fmax(md, fabs(red[q.lay.off_hpp + 21 * f + 6 * r - r * (r - 1) / 2]));
        rec->chi = red[q.lay.off_chi];
        rec->max_diag = md;
        return;
    }
    if (rec->solved == 0.) {
        rec->temp_chi = 1.7976931348623157e308;
        rec->scale = 0.;
        return;
    }
    double sc = 0., chi = 0.;
    for (int s = 0; s < n_slabs; s++) {
        sc += slabs[2 * s];
        chi += slabs[2 * s + 1];
    }
    rec->temp_chi = chi;
    rec->scale = sc + rec->scale;
}

// the final e^T e of every observation (no kernel applied)
__global__ __launch_bounds__(256) void bw_obs_chi2_kernel(BwProblem q, const double *__restrict__ poses, const double *__restrict__ X,
                                                          double *__restrict__ out)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= q.n_points)
        return;
    const double Xp[3] = {X[3 * (size_t)p], X[3 * (size_t)p + 1], X[3 * (size_t)p + 2]};
    for (int o = q.obs_start[p]; o < q.obs_start[p + 1]; o++) {
        double e2;
        bw_chi(poses + 12 * q.obs_pose[o], Xp, q.obs_uvr[3 * (size_t)o], q.obs_uvr[3 * (size_t)o + 1], q.obs_uvr[3 * (size_t)o + 2],
               q.cam, &e2);
        out[o] = e2;
    }
}

size_t bw_align(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

}  // namespace

extern "C" void svo_ba_window_default_params(svo_ba_window_params *p)
{
    if (!p)
        return;
    p->fx = p->fy = 718.856;  // include/visualSLAM.h:82-87 (KITTI 00-02), as svo_vo_default_params
    p->cx = 607.1928;
    p->cy = 185.2157;
    p->bf = 718.856 * 0.54;
    p->iterations = 10;
    p->huber_mono = 0.;
    p->huber_stereo = 0.;
}

#define BW_REFUSE(why)                                \
    do {                                              \
        svo_set_error("svo_ba_window: %s", (why));    \
        return SVO_ERR_ARG;                           \
    } while (0)

extern "C" int svo_ba_window(svo_ctx *ctx, const svo_ba_window_params *p, int n_poses, double *poses12, const uint8_t *pose_fixed,
                             int n_points, const float *pts3d, const int *obs_start, const int *obs_pose, const float *obs_uvr,
                             double *pts3d_out, double *obs_chi2_out, double *info, int mem)
{
    plan::Plan pl;
    if (const char *why = plan::check_scalars(p, n_poses, poses12, pose_fixed, n_points, pts3d, obs_start, obs_pose, obs_uvr, mem, &pl)) {
        svo_set_error("svo_ba_window: %s", why);
        return std::strstr(why, "at most 2^") ? SVO_ERR_CAPACITY : SVO_ERR_ARG;
    }
    if (mem == SVO_MEM_DEVICE && !ctx)
        BW_REFUSE("ctx must not be null");
    // the CSR arrays on the host: the caller's own, or a copy of the device's
    const int *h_start = obs_start, *h_pose = obs_pose;
    const float *h_uvr = obs_uvr;
    if (mem == SVO_MEM_DEVICE) {
        SVO_HIP(hipSetDevice(ctx->device));
        const size_t b_start = bw_align((size_t)(n_points + 1) * 4);
        if (ctx->ba_win_host.size() < b_start)
            ctx->ba_win_host.resize(b_start);
        SVO_HIP(hipMemcpyAsync(ctx->ba_win_host.data(), obs_start, (size_t)(n_points + 1) * 4, hipMemcpyDeviceToHost, ctx->stream));
        int rc = svo_wait(ctx);
        if (rc)
            return rc;
        h_start = reinterpret_cast<const int *>(ctx->ba_win_host.data());
    }
    if (const char *why = plan::check_starts(n_points, h_start)) {
        svo_set_error("svo_ba_window: %s", why);
        return std::strstr(why, "at most 2^") ? SVO_ERR_CAPACITY : SVO_ERR_ARG;
    }
    const int n_obs = h_start[n_points];
    if (mem == SVO_MEM_DEVICE && n_obs > 0) {
        const size_t b_start = bw_align((size_t)(n_points + 1) * 4), b_pose = bw_align((size_t)n_obs * 4);
        if (ctx->ba_win_host.size() < b_start + b_pose + (size_t)n_obs * 12)
            ctx->ba_win_host.resize(b_start + b_pose + (size_t)n_obs * 12);
        unsigned char *h = ctx->ba_win_host.data();
        SVO_HIP(hipMemcpyAsync(h + b_start, obs_pose, (size_t)n_obs * 4, hipMemcpyDeviceToHost, ctx->stream));
        SVO_HIP(hipMemcpyAsync(h + b_start + b_pose, obs_uvr, (size_t)n_obs * 12, hipMemcpyDeviceToHost, ctx->stream));
        int rc = svo_wait(ctx);
        if (rc)
            return rc;
        h_start = reinterpret_cast<const int *>(h);
        h_pose = reinterpret_cast<const int *>(h + b_start);
        h_uvr = reinterpret_cast<const float *>(h + b_start + b_pose);
    }
    if (const char *why = plan::check_csr(p, n_poses, n_points, h_start, h_pose, h_uvr, &pl))
        BW_REFUSE(why);
    if (!ctx)
        BW_REFUSE("ctx must not be null");
    SVO_HIP(hipSetDevice(ctx->device));

    // ---- buffers: every one is sized before the first launch (growing a buffer frees it) ----
    const plan::SlabLayout lay = plan::slab_layout(pl.n_free);
    const int n_slab1 = plan::schur_slabs(n_points), n_slab2 = plan::backsub_slabs(n_points);
    const size_t b_X = bw_align((size_t)n_points * 24);
    const size_t b_pose = bw_align((size_t)plan::MAX_POSES * 96), b_red = bw_align((size_t)lay.stride * 8),
                 b_dp = bw_align((size_t)plan::MAX_DIM * 8), b_s2 = bw_align((size_t)n_slab2 * 16), b_rec = bw_align(sizeof(BwRecord));
    int rc;
    if ((rc = ctx->w_a.ensure(2 * b_X)) || (rc = ctx->w_b.ensure((size_t)n_slab1 * lay.stride * 8)) ||
        (rc = ctx->w_c.ensure(2 * b_pose + b_red + b_dp + b_s2 + b_rec)) || (rc = ctx->w_d.ensure((size_t)(n_obs > 0 ? n_obs : 1) * 8)))
        return rc;
    BwProblem q;
    q.cam = BwCam{p->fx, p->fy, p->cx, p->cy, p->bf, p->huber_mono, p->huber_stereo};
    q.n_points = n_points;
    q.n_poses = n_poses;
    q.n_free = pl.n_free;
    q.lay = lay;
    q.pts3d = pts3d;
    q.obs_start = obs_start;
    q.obs_pose = obs_pose;
    q.obs_uvr = obs_uvr;
    for (int j = 0; j < plan::MAX_POSES; j++)
        q.free_index[j] = (signed char)(j < n_poses ? pl.free_index[j] : -1);
    for (int f = 0; f < plan::MAX_FREE; f++)
        q.free_list[f] = (signed char)(f < pl.n_free ? pl.free_list[f] : 0);
    if (mem == SVO_MEM_HOST) {
        if ((rc = ctx->s_a.ensure((size_t)n_points * 12)) || (rc = ctx->s_b.ensure((size_t)(n_points + 1) * 4)) ||
            (rc = ctx->s_c.ensure((size_t)(n_obs > 0 ? n_obs : 1) * 4)) || (rc = ctx->s_d.ensure((size_t)(n_obs > 0 ? n_obs : 1) * 12)))
            return rc;
        SVO_HIP(hipMemcpyAsync(ctx->s_a.p, pts3d, (size_t)n_points * 12, hipMemcpyHostToDevice, ctx->stream));
        SVO_HIP(hipMemcpyAsync(ctx->s_b.p, obs_start, (size_t)(n_points + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
        if (n_obs > 0) {
            SVO_HIP(hipMemcpyAsync(ctx->s_c.p, obs_pose, (size_t)n_obs * 4, hipMemcpyHostToDevice, ctx->stream));
            SVO_HIP(hipMemcpyAsync(ctx->s_d.p, obs_uvr, (size_t)n_obs * 12, hipMemcpyHostToDevice, ctx->stream));
        }
        q.pts3d = ctx->s_a.as<float>();
        q.obs_start = ctx->s_b.as<int>();
        q.obs_pose = ctx->s_c.as<int>();
        q.obs_uvr = ctx->s_d.as<float>();
    }
    unsigned char *wc = ctx->w_c.as<unsigned char>();
    double *d_cur = reinterpret_cast<double *>(wc), *d_trial = reinterpret_cast<double *>(wc + b_pose);
    double *d_red = reinterpret_cast<double *>(wc + 2 * b_pose), *d_dp = reinterpret_cast<double *>(wc + 2 * b_pose + b_red);
    double *d_s2 = reinterpret_cast<double *>(wc + 2 * b_pose + b_red + b_dp);
    BwRecord *d_rec = reinterpret_cast<BwRecord *>(wc + 2 * b_pose + b_red + b_dp + b_s2);
    double *d_X = ctx->w_a.as<double>(), *d_Xn = reinterpret_cast<double *>(ctx->w_a.as<unsigned char>() + b_X);
    double *d_slabs = ctx->w_b.as<double>(), *d_oc = ctx->w_d.as<double>();
    // pinned: the record, then the poses on their way in and out
    BwRecord *h_rec = reinterpret_cast<BwRecord *>(ctx->pinned);
    double *h_poses = reinterpret_cast<double *>(reinterpret_cast<unsigned char *>(ctx->pinned) + 256);
    memcpy(h_poses, poses12, (size_t)n_poses * 96);
    SVO_HIP(hipMemcpyAsync(d_cur, h_poses, (size_t)n_poses * 96, hipMemcpyHostToDevice, ctx->stream));
    SVO_HIP(hipMemsetAsync(d_rec, 0, sizeof(BwRecord), ctx->stream));

    const size_t lds = (size_t)(lay.stride + plan::MAX_POSES * (BW_PT + 36)) * 8 + 2 * plan::MAX_POSES * 4;
    const dim3 g_red((lay.stride + 255) / 256);
    ScopedKernelTime tm(ctx, SVO_K_PNP);
    hipLaunchKernelGGL(bw_init_points_kernel, dim3((3 * n_points + 255) / 256), dim3(256), 0, ctx->stream, q.pts3d, 3 * n_points, d_X);
    // ---- the first look: chi2 and max |diag H| ----
    hipLaunchKernelGGL(bw_schur_kernel<false>, dim3(n_slab1), dim3(64), lds, ctx->stream, q, d_cur, d_X, 0., d_slabs);
    hipLaunchKernelGGL(bw_reduce_kernel, g_red, dim3(256), 0, ctx->stream, d_slabs, n_slab1, lay.stride, lay.off_max, d_red);
    hipLaunchKernelGGL(bw_record_kernel, dim3(1), dim3(64), 0, ctx->stream, q, 1, d_red, d_s2, n_slab2, d_rec);
    SVO_HIP(hipGetLastError());
    SVO_HIP(hipMemcpyAsync(h_rec, d_rec, sizeof(BwRecord), hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = svo_wait(ctx)))
        return rc;
    plan::LmState st;
    st.chi = h_rec->chi;
    st.lambda = plan::lambda_init(h_rec->max_diag);
    const double chi_first = st.chi;
    int it_run = 0, trials = 0;
    for (int it = 0; it < p->iterations; it++) {
        st.qmax = 0;
        bool bad = false;
        do {
            hipLaunchKernelGGL(bw_schur_kernel<true>, dim3(n_slab1), dim3(64), lds, ctx->stream, q, d_cur, d_X, st.lambda, d_slabs);
            hipLaunchKernelGGL(bw_reduce_kernel, g_red, dim3(256), 0, ctx->stream, d_slabs, n_slab1, lay.stride, lay.off_max, d_red);
            hipLaunchKernelGGL(bw_solve_kernel, dim3(1), dim3(256), 0, ctx->stream, q, d_red, st.lambda, d_cur, d_trial, d_dp, d_rec);
            hipLaunchKernelGGL(bw_backsub_kernel, dim3(n_slab2), dim3(plan::BLOCK), 0, ctx->stream, q, d_cur, d_trial, d_X, d_Xn, d_dp,
                               st.lambda, d_rec, d_s2);
            hipLaunchKernelGGL(bw_record_kernel, dim3(1), dim3(64), 0, ctx->stream, q, 0, d_red, d_s2, n_slab2, d_rec);
            SVO_HIP(hipGetLastError());
            SVO_HIP(hipMemcpyAsync(h_rec, d_rec, sizeof(BwRecord), hipMemcpyDeviceToHost, ctx->stream));
            if ((rc = svo_wait(ctx)))
                return rc;
            trials++;
            if (plan::lm_trial(st, h_rec->temp_chi, h_rec->scale, h_rec->solved != 0.)) {
                std::swap(d_X, d_Xn);
                std::swap(d_cur, d_trial);
            } else if (!std::isfinite(st.lambda)) {
                bad = true;
                break;
            }
        } while (st.rho < 0 && st.qmax < 10);
        it_run = it + 1;
        if (st.qmax == 10 || st.rho == 0 || bad)
            break;  // OptimizationAlgorithm::Terminate
    }
    if (obs_chi2_out && n_obs > 0) {
        hipLaunchKernelGGL(bw_obs_chi2_kernel, dim3((n_points + 255) / 256), dim3(256), 0, ctx->stream, q, d_cur, d_X, d_oc);
        SVO_HIP(hipGetLastError());
        SVO_HIP(hipMemcpyAsync(obs_chi2_out, d_oc, (size_t)n_obs * 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    SVO_HIP(hipMemcpyAsync(h_poses, d_cur, (size_t)n_poses * 96, hipMemcpyDeviceToHost, ctx->stream));
    if (pts3d_out)
        SVO_HIP(hipMemcpyAsync(pts3d_out, d_X, (size_t)n_points * 24, hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = svo_wait(ctx)))
        return rc;
    memcpy(poses12, h_poses, (size_t)n_poses * 96);
    if (info) {
        info[0] = chi_first;
        info[1] = st.chi;
        info[2] = p->iterations > 0 ? st.lambda : 0.;
        info[3] = it_run;
        info[4] = trials;
        info[5] = n_obs;
    }
    return SVO_OK;
}
