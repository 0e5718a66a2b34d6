// posegraph.hip -- SE3 pose-graph Gauss-Newton for gfx950.
//
// Replaces the g2o wrapper globalPoseGraph of include/poseGraph.h:
//   initializeGraph :69-84, augmentNode :87-111, addLoopClosure :113-126,
//   globalOptimize :128-138 (Gauss-Newton, 10 iterations, BlockSolver<6,6> + sparse
//   Cholesky, identity information), saveStructure :140-179.
// Beyond the reference: per-edge information matrices (its own `information` member, :42, whose setInformation calls are
// commented out) and loop closures that carry a measured relative pose -- a second instantiation of the linearisation,
// launched only for a graph that stores a non-identity matrix.
//
// One Gauss-Newton iteration on the context's stream (f64 throughout):
//   linearize  one thread per edge: error e = toVectorMQT(Z^-1 Xi^-1 Xj), analytic 6x6
//              Jacobians, and the edge's blocks Ji^T Ji, Ji^T Jj, Jj^T Jj, Ji^T e, Jj^T e
//              written to per-edge slots (the "per-edge 6x6 Jacobian blocks");
//   assemble   one thread per vertex: its diagonal block, gradient and chain block are summed
//              from its incident edges in edge order -- a gather, so the sum order is fixed and
//              the result reproducible (no float atomics);
//   solve      H dx = -b by a Cholesky factorisation in nested-dissection order: chain segments
//              in parallel (one wavefront each), a dense Schur complement on the separators
//              (loop-closure endpoints + every 128th vertex), back-substitution -- see below;
//   update     one thread per vertex: X <- X * fromVectorMQT(dx).
//
// The host logic is in two headers with nothing of HIP in them, each run on its own under the host sanitizers: the
// elimination structure of the solve (pg_solve_plan.hip.h) and the .g2o reader with the test of an information matrix
// (pg_g2o.hip.h); the pruning's is in pg_prune_plan.hip.h.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "pg_g2o.hip.h"
#include "pg_prune_plan.hip.h"
#include "pg_solve_plan.hip.h"
#include "svo_internal.h"
#include "wave_ops.hip.h"

namespace {

namespace psp = pg_solve_plan;
using pg_g2o::pg_tri;
using pg_g2o::q_normalize;
using pg_solve_plan::PG_MAX_SEG_CHORDS;
using pg_solve_plan::PgTerm;
using pg_solve_plan::SEG_L;
using pg_solve_plan::TB;

// ---- SE3 with unit quaternions: pose7 = tx ty tz qx qy qz qw -----------------------------------
__host__ __device__ inline void q_mul(const double *a, const double *b, double *o)
{
    const double ax = a[0], ay = a[1], az = a[2], aw = a[3], bx = b[0], by = b[1], bz = b[2], bw = b[3];
    o[0] = aw * bx + ax * bw + ay * bz - az * by;
    o[1] = aw * by - ax * bz + ay * bw + az * bx;
    o[2] = aw * bz + ax * by - ay * bx + az * bw;
    o[3] = aw * bw - ax * bx - ay * by - az * bz;
}
__host__ __device__ inline void q_rot(const double *q, const double *v, double *o)
{
    const double ux = q[0], uy = q[1], uz = q[2], w = q[3];
    const double cx = uy * v[2] - uz * v[1], cy = uz * v[0] - ux * v[2], cz = ux * v[1] - uy * v[0];
    const double dx = uy * cz - uz * cy, dy = uz * cx - ux * cz, dz = ux * cy - uy * cx;
    o[0] = v[0] + 2 * (w * cx + dx);
    o[1] = v[1] + 2 * (w * cy + dy);
    o[2] = v[2] + 2 * (w * cz + dz);
}
__host__ __device__ inline void se3_mul(const double *A, const double *B, double *O)
{
    double t[3], q[4];
    q_rot(A + 3, B, t);
    for (int i = 0; i < 3; i++)
        t[i] += A[i];
    q_mul(A + 3, B + 3, q);
    for (int i = 0; i < 3; i++)
        O[i] = t[i];
    for (int i = 0; i < 4; i++)
        O[3 + i] = q[i];
}
__host__ __device__ inline void se3_inv(const double *A, double *O)
{
    const double qi[4] = {-A[3], -A[4], -A[5], A[6]};
    double t[3];
    q_rot(qi, A, t);
    for (int i = 0; i < 3; i++)
        O[i] = -t[i];
    for (int i = 0; i < 4; i++)
        O[3 + i] = qi[i];
}
__device__ inline void q_to_R(const double *q, double *R)
{
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    R[0] = 1 - 2 * (y * y + z * z);
    R[1] = 2 * (x * y - z * w);
    R[2] = 2 * (x * z + y * w);
    R[3] = 2 * (x * y + z * w);
    R[4] = 1 - 2 * (x * x + z * z);
    R[5] = 2 * (y * z - x * w);
    R[6] = 2 * (x * z - y * w);
    R[7] = 2 * (y * z + x * w);
    R[8] = 1 - 2 * (x * x + y * y);
}

// per-edge outputs: 3 blocks + 2 gradients + chi2, one record of EO_FIELDS doubles per edge
// (EO_W: the robust weight of the edge, written by the robust instantiations only)
enum { EO_HII = 0, EO_HIJ = 36, EO_HJJ = 72, EO_BI = 108, EO_BJ = 114, EO_CHI2 = 120, EO_W = 121, EO_FIELDS = 122 };

// The robust kernels at c = chi2 of an edge: the weight w = rho'(c) that scales the edge's information, and rho itself.  g2o's
// robust_kernel_impl.h and Open3D's line process, from memory -- verify (include/svo.h has the table).  DCS: g2o's weight s^2 is not
// the derivative of its rho = s^2 c (s depends on c); it is reproduced as it stands.  delta is finite and positive (checked on entry).
__device__ inline double pg_robust_weight(int kind, double delta, double c, double *rho)
{
    double w = 1., r = c;
    if (kind == SVO_PG_ROBUST_HUBER) {
        if (c > delta * delta) {
            const double sq = sqrt(c);
            w = delta / sq;
            r = 2. * delta * sq - delta * delta;
        }
    } else if (kind == SVO_PG_ROBUST_CAUCHY) {
        const double d2 = delta * delta, aux = 1. + c / d2;
        w = 1. / aux;
        r = d2 * svo_log(aux);
    } else if (kind == SVO_PG_ROBUST_DCS) {
        const double sc = 2. * delta / (delta + c);
        if (sc < 1.) {
            w = sc * sc;
            r = w * c;
        }
    } else if (kind == SVO_PG_ROBUST_GEMAN_MCCLURE) {
        const double l = delta / (delta + c);
        w = l * l;
        r = delta * c / (delta + c);
    }
    *rho = r;
    return w;
}

// WEIGHTED = false: identity information, chi2 = e^T e, H = J^T J -- the kernel of every graph that stores no information.
// WEIGHTED = true: a second instantiation, launched only for a graph with at least one stored information matrix:
// `info` holds 21 doubles per edge (pg_tri), chi2 = e^T (Om e), b = J^T (Om e), H = J^T (Om J).  Om J is never held as a
// whole: per output column q the six values w = Om J[:, q] are formed and dotted with the columns of Ji and Jj.
// ROBUST = true: two more instantiations, launched only for a graph that stores at least one robust kernel: (rkind, rdelta) per
// edge, w = rho'(chi) scales the FINISHED blocks and gradients as they are stored (w == 1: times 1.0, the other instantiation's
// bits; a diagonal block's two mirrored entries are the same product) and goes to EO_W.  chi2 stays the unweighted e^T Om e.
template <bool WEIGHTED, bool ROBUST>
__global__ __launch_bounds__(128) void pg_linearize_kernel(const double *__restrict__ pose, const int *__restrict__ efrom,
                                                           const int *__restrict__ eto, const double *__restrict__ meas,
                                                           int ne, double *__restrict__ out, double *__restrict__ part,
                                                           unsigned *__restrict__ ticket, double *__restrict__ chi2_out,
                                                           const double *__restrict__ info,
                                                           const int *__restrict__ rkind,
                                                           const double *__restrict__ rdelta)
{
    __shared__ double s_chi[128];
    __shared__ bool s_last;
    const int e_raw = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = e_raw < ne;
    const int e = live ? e_raw : ne - 1;  // the threads past the end redo the last edge and write nothing
    const double *Xi = pose + 7 * efrom[e], *Xj = pose + 7 * eto[e], *Z = meas + 7 * e;
    double A[7], Xi_inv[7], B[7], E[7];
    se3_inv(Z, A);
    se3_inv(Xi, Xi_inv);
    se3_mul(Xi_inv, Xj, B);
    se3_mul(A, B, E);
    const double s = E[6] < 0 ? -1. : 1.;
    const double err[6] = {E[0], E[1], E[2], s * E[3], s * E[4], s * E[5]};
    double chi = 0;
    double Om[WEIGHTED ? 21 : 1], we[6];  // we = Om e
    if constexpr (WEIGHTED) {
#pragma unroll
        for (int k = 0; k < 21; k++)
            Om[k] = info[21 * (size_t)e + k];
#pragma unroll
        for (int r = 0; r < 6; r++) {
            double acc = 0;
#pragma unroll
            for (int k = 0; k < 6; k++)
                acc += Om[pg_tri(r, k)] * err[k];
            we[r] = acc;
        }
#pragma unroll
        for (int k = 0; k < 6; k++)
            chi += err[k] * we[k];
    } else {
#pragma unroll
        for (int k = 0; k < 6; k++)
            chi += err[k] * err[k];
    }
    // chi2 of the whole graph rides along: a fixed tree per workgroup, and the workgroup that finishes last adds the
    // workgroups' sums in index order (the ticket resets itself for the next launch) -- no launch of its own, and
    // BEFORE the blocks are formed and stored, so that the fence has one store to wait for
    s_chi[threadIdx.x] = live ? chi : 0.;
    __syncthreads();
    for (int off = 64; off >= 1; off >>= 1) {
        if ((int)threadIdx.x < off)
            s_chi[threadIdx.x] += s_chi[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        __hip_atomic_store(&part[blockIdx.x], s_chi[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __threadfence();
        s_last = atomicAdd(ticket, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (s_last) {
        __threadfence();
        double sum = 0;  // (thread 0's)
        for (unsigned base = 0; base < gridDim.x; base += 128) {  // the sums arrive 128 at a time, thread 0 adds them in order
            const unsigned k = base + threadIdx.x;
            s_chi[threadIdx.x] =
                k < gridDim.x ? __hip_atomic_load(&part[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.;
            __syncthreads();
            if (threadIdx.x == 0)
                for (unsigned q = 0; q < 128 && base + q < gridDim.x; q++)
                    sum += s_chi[q];
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            *chi2_out = sum;
            *ticket = 0;
        }
    }
    double Ji[36], Jj[36], Re[9], Ra[9];
#pragma unroll
    for (int k = 0; k < 36; k++) {
        Ji[k] = 0;
        Jj[k] = 0;
    }
    q_to_R(E + 3, Re);
    q_to_R(A + 3, Ra);
    {  // Xj <- Xj * D:  d te/du = Re,  d vec(qe)/dv = w I + [u]x
        const double ux = E[3], uy = E[4], uz = E[5], w = E[6];
        const double Q[9] = {w, -uz, uy, uz, w, -ux, -uy, ux, w};
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int c = 0; c < 3; c++) {
                Jj[6 * r + c] = Re[3 * r + c];
                Jj[6 * (3 + r) + 3 + c] = s * Q[3 * r + c];
            }
    }
    {  // Xi <- Xi * D:  d te/du = -Ra,  d te/dv = 2 Ra [tb]x,  d vec/dv = -[L(qa) R(qb)]_xyz
        const double tb[3] = {B[0], B[1], B[2]};
        const double Tx[9] = {0, -tb[2], tb[1], tb[2], 0, -tb[0], -tb[1], tb[0], 0};
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int c = 0; c < 3; c++) {
                Ji[6 * r + c] = -Ra[3 * r + c];
                double acc = 0;
#pragma unroll
                for (int k = 0; k < 3; k++)
                    acc += Ra[3 * r + k] * Tx[3 * k + c];
                Ji[6 * r + 3 + c] = 2. * acc;
            }
        const double aw = A[6], ax = A[3], ay = A[4], az = A[5];
        const double bw = B[6], bx = B[3], by = B[4], bz = B[5];
        const double L[16] = {aw, -ax, -ay, -az, ax, aw, -az, ay, ay, az, aw, -ax, az, -ay, ax, aw};
        const double Rm[16] = {bw, -bx, -by, -bz, bx, bw, bz, -by, by, -bz, bw, bx, bz, by, -bx, bw};
#pragma unroll
        for (int r = 1; r < 4; r++)
#pragma unroll
            for (int c = 1; c < 4; c++) {
                double acc = 0;
#pragma unroll
                for (int k = 0; k < 4; k++)
                    acc += L[4 * r + k] * Rm[4 * k + c];
                Ji[6 * (3 + r - 1) + 3 + c - 1] = -s * acc;
            }
    }
    if (live) {
        double *o = out + (size_t)e * EO_FIELDS;
        o[EO_CHI2] = chi;
        double rw = 1.;  // (read by the robust instantiations only)
        if constexpr (ROBUST) {
            double rho;
            rw = pg_robust_weight(rkind[e], rdelta[e], chi, &rho);
            o[EO_W] = rw;
        }
        if constexpr (WEIGHTED) {
#pragma unroll
            for (int p = 0; p < 6; p++) {
                double si = 0, sj = 0;
#pragma unroll
                for (int k = 0; k < 6; k++) {
                    si += Ji[6 * k + p] * we[k];
                    sj += Jj[6 * k + p] * we[k];
                }
                o[EO_BI + p] = ROBUST ? si * rw : si;
                o[EO_BJ + p] = ROBUST ? sj * rw : sj;
            }
#pragma unroll
            for (int q = 0; q < 6; q++) {
                double wi[6], wj[6];  // Om Ji[:, q], Om Jj[:, q]
#pragma unroll
                for (int r = 0; r < 6; r++) {
                    double a = 0, b = 0;
#pragma unroll
                    for (int k = 0; k < 6; k++) {
                        a += Om[pg_tri(r, k)] * Ji[6 * k + q];
                        b += Om[pg_tri(r, k)] * Jj[6 * k + q];
                    }
                    wi[r] = a;
                    wj[r] = b;
                }
#pragma unroll
                for (int p = 0; p < 6; p++) {
                    double a = 0, b = 0, c = 0;
#pragma unroll
                    for (int k = 0; k < 6; k++) {
                        a += Ji[6 * k + p] * wi[k];
                        b += Ji[6 * k + p] * wj[k];
                        c += Jj[6 * k + p] * wj[k];
                    }
                    o[EO_HIJ + 6 * p + q] = ROBUST ? b * rw : b;
                    // the diagonal blocks are symmetric: the upper triangle is computed, the lower mirrors it bit for bit
                    if (p <= q) {
                        o[EO_HII + 6 * p + q] = ROBUST ? a * rw : a;
                        o[EO_HJJ + 6 * p + q] = ROBUST ? c * rw : c;
                        if (p < q) {
                            o[EO_HII + 6 * q + p] = ROBUST ? a * rw : a;
                            o[EO_HJJ + 6 * q + p] = ROBUST ? c * rw : c;
                        }
                    }
                }
            }
        } else
#pragma unroll
        for (int p = 0; p < 6; p++) {
            double si = 0, sj = 0;
#pragma unroll
            for (int k = 0; k < 6; k++) {
                si += Ji[6 * k + p] * err[k];
                sj += Jj[6 * k + p] * err[k];
            }
            o[EO_BI + p] = ROBUST ? si * rw : si;
            o[EO_BJ + p] = ROBUST ? sj * rw : sj;
#pragma unroll
            for (int q = 0; q < 6; q++) {
                double a = 0, b = 0, c = 0;
#pragma unroll
                for (int k = 0; k < 6; k++) {
                    a += Ji[6 * k + p] * Ji[6 * k + q];
                    b += Ji[6 * k + p] * Jj[6 * k + q];
                    c += Jj[6 * k + p] * Jj[6 * k + q];
                }
                o[EO_HII + 6 * p + q] = ROBUST ? a * rw : a;
                o[EO_HIJ + 6 * p + q] = ROBUST ? b * rw : b;
                o[EO_HJJ + 6 * p + q] = ROBUST ? c * rw : c;
            }
        }
    }
}

// chi2, w and rho of every edge at the current estimates, no blocks: one thread per edge, the error and chi2 by the operations of
// pg_linearize_kernel in its order (so chi2 and w are that kernel's bits).  For svo_pg_edge_residuals and svo_pg_prune_edges.
// rkind == nullptr: no edge carries a kernel.  res: chi2 [ne] | w [ne] | rho [ne].
template <bool WEIGHTED>
__global__ __launch_bounds__(128) void pg_edge_eval_kernel(const double *__restrict__ pose, const int *__restrict__ efrom,
                                                           const int *__restrict__ eto, const double *__restrict__ meas,
                                                           int ne, const double *__restrict__ info,
                                                           const int *__restrict__ rkind, const double *__restrict__ rdelta,
                                                           double *__restrict__ res)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= ne)
        return;
    const double *Xi = pose + 7 * efrom[e], *Xj = pose + 7 * eto[e], *Z = meas + 7 * e;
    double A[7], Xi_inv[7], B[7], E[7];
    se3_inv(Z, A);
    se3_inv(Xi, Xi_inv);
    se3_mul(Xi_inv, Xj, B);
    se3_mul(A, B, E);
    const double s = E[6] < 0 ? -1. : 1.;
    const double err[6] = {E[0], E[1], E[2], s * E[3], s * E[4], s * E[5]};
    double chi = 0;
    if constexpr (WEIGHTED) {
        double we[6];
#pragma unroll
        for (int r = 0; r < 6; r++) {
            double acc = 0;
#pragma unroll
            for (int k = 0; k < 6; k++)
                acc += info[21 * (size_t)e + pg_tri(r, k)] * err[k];
            we[r] = acc;
        }
#pragma unroll
        for (int k = 0; k < 6; k++)
            chi += err[k] * we[k];
    } else {
#pragma unroll
        for (int k = 0; k < 6; k++)
            chi += err[k] * err[k];
    }
    double rho = chi;
    const double w = rkind ? pg_robust_weight(rkind[e], rdelta[e], chi, &rho) : 1.;
    res[e] = chi;
    res[(size_t)ne + e] = w;
    res[2 * (size_t)ne + e] = rho;
}

// ---- the linear solve  H dx = -b --------------------------------------------------------------
//
// Unknown block b = vertex b+1 (vertex 0 is fixed).  H is block tridiagonal along the odometry
// chain plus one block pair per loop-closure edge ("chord").  A Cholesky factorisation in time
// order is one serial chain of nb block steps with the fill of every chord on top; instead the
// rows are ordered by ONE level of nested dissection:
//   separators  = the endpoints of all chords + every SEG_L-th row;
//   segments    = the runs of rows between consecutive separators: independent block-tridiagonal
//                 systems, factorised and solved by one wavefront each, all in parallel;
//   reduced system = the Schur complement on the separators (block tridiagonal in separator
//                 order + the chord blocks), assembled by gathers in a fixed order and solved by a
//                 blocked dense Cholesky (48-wide tiles, many workgroups per step);
//   back-substitution of the segment interiors, one thread per unknown.
// This is still a Cholesky factorisation of H (under a symmetric block permutation), so it is as
// stable as the time-ordered one, and every sum has a fixed order (no float atomics).
//
// Segment rows a..z with left separator l = a-1 and right separator r = z+1 (either may be
// missing at the ends of the chain).  With C_b = H[b+1][b]:
//   T x_seg + E_a C_l x_l + E_z C_z^T x_r = r_seg   =>   x_seg = y - Wl x_l - Wr x_r,
//   y = T^-1 r_seg,  Wl = T^-1 E_a C_l,  Wr = T^-1 E_z C_z^T.

// (PG_MAX_SEG_CHORDS, SEG_L and TB: pg_solve_plan.hip.h)

// A workgroup barrier that orders LDS traffic only.  __syncthreads() on gfx9 also waits for every global load and store of
// the wave (one counter for both, and a release fence has to wait for the stores): loads asked for early would be drained
// at the next barrier.  The kernels below exchange data between their waves through LDS alone.
__device__ __forceinline__ void lds_barrier()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// assemble: one thread per block row AND entry (36 of the diagonal block, 36 of the chain block, 6 of the gradient): the
// 78 threads of a row read consecutive doubles of an edge's record and write consecutive doubles of the row's blocks.
// (One thread per row with 78 sums in registers: 4540 threads and three dependent rounds of scattered loads, 15.7 us.)
// Incident edges of vertex v are inc[incptr[v] .. incptr[v+1]) = edge*2 + role (role 0: v is the edge's `from`, 1: `to`),
// ascending in edge index, so every sum has a fixed order.
//   Dg[b]  = sum of the vertex's diagonal blocks,  rneg[b] = -(sum of its gradients),
//   Cc[b]  = H[b+1][b], the blocks of the edges between vertices b+1 and b+2.
constexpr int PG_ASM_ROWS = 3;  // rows per workgroup: 3 x 78 = 234 threads
__global__ __launch_bounds__(PG_ASM_ROWS * 78) void pg_assemble_kernel(int nb, const int *__restrict__ incptr,
                                                                       const int *__restrict__ inc,
                                                                       const int *__restrict__ efrom,
                                                                       const int *__restrict__ eto,
                                                                       const double *__restrict__ eo,
                                                                       double *__restrict__ Dg, double *__restrict__ Cc,
                                                                       double *__restrict__ rneg)
{
    const int b = blockIdx.x * PG_ASM_ROWS + threadIdx.x / 78, k = threadIdx.x % 78;
    if (b >= nb)
        return;
    const int v = b + 1;
    double acc = 0;
    for (int t = incptr[v]; t < incptr[v + 1]; t++) {
        const int e = inc[t] >> 1, role = inc[t] & 1;
        const double *o = eo + (size_t)e * EO_FIELDS;
        if (k < 36)
            acc += o[(role ? EO_HJJ : EO_HII) + k];
        else if (k >= 72)
            acc += o[(role ? EO_BJ : EO_BI) + (k - 72)];
        else if ((role ? efrom[e] : eto[e]) == v + 1) {
            // block(v+1, v) = J_{v+1}^T J_v: v = `to` (role 1): Ji^T Jj as stored; v = `from`: its transpose
            const int p = (k - 36) / 6, q = (k - 36) - 6 * p;
            acc += o[EO_HIJ + (role ? 6 * p + q : 6 * q + p)];
        }
    }
    if (k < 36)
        Dg[(size_t)b * 36 + k] = acc;
    else if (k < 72)
        Cc[(size_t)b * 36 + (k - 36)] = acc;
    else
        rneg[(size_t)b * 6 + (k - 72)] = -acc;
}

// 6x6 Cholesky S = L L^T and the inverse of L, by the 64 lanes of one wave on LDS arrays
// (sS is destroyed).  Returns false (wave-uniform) at a non-positive pivot.
// The pivots' reciprocal square roots come from v_rsq_f64 and two Newton steps (to the last bits of a double) and
// are kept: L_kk = pivot * rsqrt, the column scales and the forward substitution of the inverse multiply by them.  A
// square root and a division per pivot and a division per row of the inverse were two thirds of this routine, and this
// routine is the serial chain of the segments (a call per block row) and of the separator tiles (eight per tile).
__device__ __forceinline__ double pg_readlane(double v, int src)  // src: a compile-time constant after unrolling
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), src);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
    return __hiloint2double(hi, lo);
}
// Row r of the matrix lives in the registers of lane r (six lanes work, the others shadow lane 0); what a lane needs of
// another row arrives through v_readlane, so the six pivot steps and the forward substitution of the inverse touch
// neither LDS nor a barrier.
// The two halves, on registers: the factor (row `row` of L in a[], the pivots' reciprocal square roots in rinv[]) ...
__device__ __forceinline__ bool wave_chol6_regs(const double *sS, int lane, double (&a)[6], double (&rinv)[6])
{
    const int row = lane < 6 ? lane : 0;
#pragma unroll
    for (int c = 0; c < 6; c++)
        a[c] = sS[6 * row + c];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 6; k++) {
        const double piv = pg_readlane(a[k], k);
        if (!(piv > 0))
            ok = false;
        double y = __builtin_amdgcn_rsq(piv);
        const double hp = 0.5 * piv;
        y = y * (1.5 - hp * y * y);
        y = y * (1.5 - hp * y * y);
        rinv[k] = y;
        const double lk = row == k ? piv * y : a[k] * y;  // L[row][k] (rows >= k)
        a[k] = lk;
#pragma unroll
        for (int j = 0; j < 6; j++)
            if (j > k)
                a[j] -= lk * pg_readlane(lk, j);  // S[row][j] -= L[row][k] L[j][k]; used for j <= row only
    }
    return ok;
}
// ... and column `row` of L^-1 by forward substitution (x[r] = L^-1[r][row])
__device__ __forceinline__ void wave_inv6_regs(const double (&a)[6], const double (&rinv)[6], int lane, double (&x)[6])
{
    const int row = lane < 6 ? lane : 0;
#pragma unroll
    for (int r = 0; r < 6; r++) {
        double sacc = r == row ? 1. : 0.;
#pragma unroll
        for (int k = 0; k < 6; k++)
            if (k < r)
                sacc -= pg_readlane(a[k], r) * (k >= row ? x[k] : 0.);
        x[r] = r < row ? 0. : sacc * rinv[r];
    }
}
template <bool WANT_L = true>
__device__ inline bool wave_chol6_inv(double *sS, double *sL, double *sLi, int lane)
{
    double a[6], rinv[6], x[6];
    const bool ok = wave_chol6_regs(sS, lane, a, rinv);
    wave_inv6_regs(a, rinv, lane, x);
    if (lane < 6) {  // (sLi may be sS: every lane has read its row long ago)
        if (WANT_L) {
#pragma unroll
            for (int c = 0; c < 6; c++)
                sL[6 * lane + c] = c <= lane ? a[c] : 0.;
        }
#pragma unroll
        for (int r = 0; r < 6; r++)
            sLi[6 * r + lane] = x[r];
    }
    svo::wave_lds_fence();
    return ok;
}

// -DPG_STAMPS: thread 0 of the first tile's workgroups leaves the 100 MHz clock at the phase boundaries (tools/pg_quick.sh)
#ifdef PG_STAMPS
__device__ long long pg_dbg[128];
__device__ int pg_dbg_claim;
#define PGSTAMP(k)                                                                                                     \
    do {                                                                                                               \
        if (tid == 0 && dbg)                                                                                           \
            pg_dbg[k] = wall_clock64();                                                                                \
    } while (0)
#else
#define PGSTAMP(k) (void)dbg
#endif
// A segment = a block-tridiagonal system T X = B with 13 right-hand sides  B = [r | E_a H[a][a-1] | E_z H[z][z+1]],
// X = [y | Wl | Wr].  Solved by BLOCK CYCLIC REDUCTION in LDS, one workgroup of 16 waves per segment: at level l (stride
// s = 2^l) the rows q = s, 3s, 5s, ... (1-based) are eliminated -- all of them at once, a wave per row -- into their
// neighbours q - s and q + s, which stay; log2(n) + 1 levels down, the same up for the substitution.  (Rounds 1-3 walked
// a segment's rows one after the other, from both ends towards the middle: a serial chain of n / 2 block rows of
// ~2.3 us, 170 us for the 100-row segments of a KITTI-sized graph; the levels are 7 + 7 steps of ~1-2 us.)  It is still a
// Cholesky factorisation of T under a symmetric permutation (odd-even nested dissection): Schur complements of positive
// definite blocks, every sum in a fixed order.
//   eliminate q:  D_q = L L^T;  G-_q = L^-1 H[q][q-s],  G+_q = L^-1 H[q][q+s],  GB_q = L^-1 B_q
//   into p = q -/+ s:  D_p -= G^T G,  B_p -= G^T GB,  and the new coupling  H[p+2s][p] = -G+_{p+s}^T G-_{p+s}
//   substitute:  X_q = L^-T (GB_q - G-_q X_{q-s} - G+_q X_{q+s})
// Row slot in LDS (doubles): D -> L^-1 [36] | F = H[q+s][q] -> G+ [36] | G- [36] | B -> GB -> X [6 x 13].
constexpr int BCR_ROW = 186, BCR_F = 36, BCR_GM = 72, BCR_B = 108, BCR_WAVES = 16;
constexpr int BCR_MAX_ROWS = (160 * 1024 - 256) / (BCR_ROW * 8);  // 110 rows of LDS

// One 6 x 6 block per LANE: the same Cholesky + inverse as wave_chol6_inv, operation for operation (the results are
// bit-identical), on the packed lower triangle in a lane's registers.  For the first levels of a long segment, where there
// are more rows to eliminate than waves: 64 blocks in the time of one.  D (row-major) at `blk` becomes L^-1.
__device__ inline bool lane_chol6_inv(double *blk)
{
    double a[21], x[21], rinv[6];
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = 0; j <= i; j++)
            a[i * (i + 1) / 2 + j] = blk[6 * i + j];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 6; k++) {
        const double piv = a[k * (k + 1) / 2 + k];
        if (!(piv > 0))
            ok = false;
        double y = __builtin_amdgcn_rsq(piv);
        const double hp = 0.5 * piv;
        y = y * (1.5 - hp * y * y);
        y = y * (1.5 - hp * y * y);
        rinv[k] = y;
        a[k * (k + 1) / 2 + k] = piv * y;
#pragma unroll
        for (int i = k + 1; i < 6; i++)
            a[i * (i + 1) / 2 + k] = a[i * (i + 1) / 2 + k] * y;
#pragma unroll
        for (int j = k + 1; j < 6; j++)
#pragma unroll
            for (int i = j; i < 6; i++)
                a[i * (i + 1) / 2 + j] -= a[i * (i + 1) / 2 + k] * a[j * (j + 1) / 2 + k];
    }
#pragma unroll
    for (int j = 0; j < 6; j++)
#pragma unroll
        for (int r = j; r < 6; r++) {
            double sacc = r == j ? 1. : 0.;
#pragma unroll
            for (int k = j; k < r; k++)
                sacc -= a[r * (r + 1) / 2 + k] * x[k * (k + 1) / 2 + j];
            x[r * (r + 1) / 2 + j] = sacc * rinv[r];
        }
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = 0; j < 6; j++)
            blk[6 * i + j] = j <= i ? x[i * (i + 1) / 2 + j] : 0.;
    return ok;
}

// The workgroups past the segments clear the reduced (separator) matrix for the gather that follows -- identity on the
// padded diagonal, zeros elsewhere -- beside the segments instead of in a launch of its own.
constexpr int PG_CLEAR_WGS = 48;
// A closure with only ONE endpoint among the separators leaves its other endpoint j inside a segment, coupled to that
// separator by the edge's block H[j][i]: six more right-hand-side columns E_j H[j][i], solved in a pass of their own
// over the factor that is in LDS anyway (no factorisation, six columns down and up) -> Wc, the segment's third W.
struct PgSegChords {
    const int *cptr;   // [nseg + 1] a segment's couplings in the arrays below
    const int *lrow;   // the endpoint's row within the segment
    const int *edge;   // the closure's edge
    const int *tr;     // 0: the endpoint is the edge's `from` (block Hij), 1: its `to` (Hij^T)
    const int *wbase;  // first 6 x 6 block of this coupling's Wc (one block per row of the segment)
};
__global__ __launch_bounds__(BCR_WAVES * 64) void pg_segment_kernel(int nb, int nseg, const int *__restrict__ seg_start,
                                                                    const int *__restrict__ seg_len,
                                                                    const double *__restrict__ Dg,
                                                                    const double *__restrict__ Cc,
                                                                    const double *__restrict__ rneg,
                                                                    double *__restrict__ Y, double *__restrict__ Wl,
                                                                    double *__restrict__ Wr, int *__restrict__ status,
                                                                    double *__restrict__ R, int ldr, int n_used,
                                                                    double *__restrict__ rR, PgSegChords ch,
                                                                    const double *__restrict__ eo, double *__restrict__ Wc)
{
    if ((int)blockIdx.x >= nseg) {
        const size_t total = (size_t)ldr * ldr, step = (size_t)(gridDim.x - nseg) * BCR_WAVES * 64;
        for (size_t t = (size_t)(blockIdx.x - nseg) * BCR_WAVES * 64 + threadIdx.x; t < total; t += step) {
            const int r = (int)(t / ldr), c = (int)(t - (size_t)r * ldr);
            R[t] = (r == c && r >= n_used) ? 1. : 0.;
            if (t < (size_t)ldr)
                rR[t] = 0.;
        }
        return;
    }
    extern __shared__ double sm[];
    __shared__ int s_fail;
    // which of the separator columns of a row's right-hand side are not structurally zero (bit 0: the left separator's
    // six, bit 1: the right one's).  They start at the segment's first / last row and spread by one row that stays per
    // level; on the way down only those rows carry them (on the way up every row's X is dense).
    __shared__ unsigned char s_cols[BCR_MAX_ROWS + 2];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    constexpr int NT = BCR_WAVES * 64;
    const int a = seg_start[blockIdx.x], n = seg_len[blockIdx.x], z = a + n - 1;
    const bool has_l = a > 0, has_r = z < nb - 1;
    if (tid == 0)
        s_fail = 0;
#ifdef PG_STAMPS
    __shared__ int s_dbg;
    if (tid == 0)
        s_dbg = n >= 96 && atomicCAS(&pg_dbg_claim, 0, 1) == 0;
    __syncthreads();
    const bool dbg = s_dbg != 0;
#else
    const bool dbg = false;
#endif
    PGSTAMP(70);
    if (tid < n)
        s_cols[tid] = (unsigned char)((tid == 0 && has_l ? 1 : 0) | (tid == n - 1 && has_r ? 2 : 0));
    {  // D and F: the segment's rows are contiguous in Dg / Cc; four loads in flight per thread and array
        const double *gd = Dg + (size_t)a * 36, *gc = Cc + (size_t)a * 36;
        const int tot = n * 36;
        for (int e0 = tid; e0 < tot; e0 += 4 * NT) {
            double vd[4], vc[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int e = e0 + u * NT;
                vd[u] = e < tot ? gd[e] : 0.;
                vc[u] = e < tot - 36 ? gc[e] : 0.;  // H[b+1][b]; the last row's coupling leaves the segment
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int e = e0 + u * NT;
                if (e < tot) {
                    const int p = e / 36, k = e - 36 * p;
                    sm[p * BCR_ROW + k] = vd[u];
                    sm[p * BCR_ROW + BCR_F + k] = vc[u];
                }
            }
        }
        for (int e = tid; e < n * 78; e += NT) {  // B = [r | H[a][a-1] in the first row | H[z][z+1] in the last]
            const int p = e / 78, k = e - 78 * p, r = k / 13, c = k - 13 * r;
            double v = 0.;
            if (c == 0)
                v = rneg[(size_t)(a + p) * 6 + r];
            else if (c < 7) {
                if (p == 0 && has_l)
                    v = Cc[(size_t)(a - 1) * 36 + 6 * r + (c - 1)];
            } else if (p == n - 1 && has_r)
                v = Cc[(size_t)z * 36 + 6 * (c - 7) + r];  // Cc[z]^T
            sm[p * BCR_ROW + BCR_B + k] = v;
        }
    }
    __syncthreads();
    PGSTAMP(71);
    int levels = 0;
    auto forward = [&]() -> bool {
    levels = 0;
    for (int s = 1; s <= n; s <<= 1, levels++) {
        // ---- eliminate the rows q = s (2 t + 1): factor, and the products with L^-1 ----
        const int cnt = (n / s + 1) / 2;
        const bool by_lane = cnt > BCR_WAVES;  // more rows than waves: a lane per block first, the products after
        if (by_lane) {
            if (tid < cnt) {
                const int q = s * (2 * tid + 1);
                if (!lane_chol6_inv(sm + (q - 1) * BCR_ROW)) {
                    atomicMax(status, a + q);  // 1 + block row
                    s_fail = 1;
                }
            }
            lds_barrier();
            if (s_fail)
                return false;
        }
        for (int t = wave; t < cnt; t += BCR_WAVES) {
            const int q = s * (2 * t + 1);
            double *Q = sm + (q - 1) * BCR_ROW;
            const bool hl = q > s, hr = q + s <= n;
            if (!by_lane && !wave_chol6_inv<false>(Q, nullptr, Q, lane)) {
                if (lane == 0) {
                    atomicMax(status, a + q);
                    s_fail = 1;
                }
                continue;
            }
            const int cols = s_cols[q - 1];
            const double *Fl = sm + (hl ? q - s - 1 : q - 1) * BCR_ROW + BCR_F;  // H[q][q-s], kept by the left neighbour
            // out[i][.] = sum_u Linv[i][u] src[u * st]  (Linv is lower triangular with zeros above).  Every lane runs the
            // SAME code on its own (i, src, st, dst): round 0: G- (36 lanes) and 28 entries of G+; round 1: G+'s other 8,
            // GB's first column (6), the left separator's columns (36, where the row carries them); round 2, for the rare
            // row that carries the right separator's columns: those 36.
            const int rounds = cols & 2 ? 3 : 2;
            double out[3];
            int dsts[3];
#pragma unroll
            for (int r = 0; r < 3; r++) {
                int i = 0, st = 1, dst = -1;
                const double *src = Q;
                if (r == 0) {
                    if (lane < 36) {
                        i = lane / 6, src = Fl + lane % 6, st = 6, dst = hl ? BCR_GM + lane : -1;
                    } else {
                        const int g = lane - 36;
                        i = g / 6, src = Q + BCR_F + 6 * (g % 6), st = 1, dst = hr ? BCR_F + g : -1;
                    }
                } else if (r == 1) {
                    if (lane < 8) {
                        const int g = 28 + lane;
                        i = g / 6, src = Q + BCR_F + 6 * (g % 6), st = 1, dst = hr ? BCR_F + g : -1;
                    } else if (lane < 14) {
                        i = lane - 8, src = Q + BCR_B, st = 13, dst = BCR_B + 13 * i;
                    } else if (lane < 50) {
                        const int g = lane - 14, c = 1 + g % 6;
                        i = g / 6, src = Q + BCR_B + c, st = 13, dst = cols & 1 ? BCR_B + 13 * i + c : -1;
                    }
                } else if (lane < 36) {
                    const int c = 7 + lane % 6;
                    i = lane / 6, src = Q + BCR_B + c, st = 13, dst = BCR_B + 13 * i + c;
                }
                double acc = 0.;
                if (r < rounds) {
#pragma unroll
                    for (int u = 0; u < 6; u++)
                        acc = fma(Q[6 * i + u], src[u * st], acc);
                } else
                    dst = -1;
                out[r] = acc;
                dsts[r] = dst;
            }
            svo::wave_lds_fence();  // F_q and B_q have been read by every lane
#pragma unroll
            for (int r = 0; r < 3; r++)
                if (dsts[r] >= 0)
                    Q[dsts[r]] = out[r];
        }
        lds_barrier();
        PGSTAMP(72 + 2 * levels);
        if (s_fail)
            return false;
        // ---- into the rows that stay, p = 2 s (t + 1): every entry of D_p, B_p and the new coupling is a lane's own ----
        const int cnt2 = n / (2 * s);
        for (int t = wave; t < cnt2; t += BCR_WAVES) {
            const int p = 2 * s * (t + 1);
            double *P = sm + (p - 1) * BCR_ROW;
            const bool hr = p + s <= n, hn = p + 2 * s <= n;
            const double *Gl = sm + (p - s - 1) * BCR_ROW;                 // the eliminated row on the left: its G+ is ours
            const double *Gr = sm + ((hr ? p + s : p - s) - 1) * BCR_ROW;  // on the right: its G-
            const int cols = s_cols[p - 1] | s_cols[p - s - 1] | (hr ? s_cols[p + s - 1] : 0);
            // out = base - sum_u A1[6 u] B1[u * st] - sum_u A2[6 u] B2[u * st]: the same code in every lane (see above);
            // round 0: D_p (36) and 28 entries of the new coupling, round 1: its other 8, B_p's first column (6), the left
            // separator's columns (36), round 2: the right separator's columns
            const int rounds = cols & 2 ? 3 : 2;
#pragma unroll
            for (int r = 0; r < 3; r++) {
                if (r >= rounds)
                    break;
                int st = 6, dst = -1;
                bool use1 = true, use2 = hr, keep = true;
                const double *A1 = Gl, *B1 = Gl, *A2 = Gl, *B2 = Gl;
                auto coupling = [&](int g) {  // H[p+2s][p][i][j] = -sum_t G+r[t][i] G-r[t][j]
                    const int i = g / 6, j = g - 6 * i;
                    A2 = Gr + BCR_F + i, B2 = Gr + BCR_GM + j, dst = hn ? BCR_F + g : -1;
                    use1 = false, use2 = hn, keep = false;
                };
                auto rhs = [&](int i, int c, bool on) {  // B_p[i][c] -= sum_t G+l[t][i] GBl[t][c] + sum_t G-r[t][i] GBr[t][c]
                    A1 = Gl + BCR_F + i, B1 = Gl + BCR_B + c, A2 = Gr + BCR_GM + i, B2 = Gr + BCR_B + c;
                    st = 13, dst = on ? BCR_B + 13 * i + c : -1;
                };
                if (r == 0) {
                    if (lane < 36) {  // D_p[i][j] -= sum_t G+l[t][i] G+l[t][j] + sum_t G-r[t][i] G-r[t][j]
                        const int i = lane / 6, j = lane - 6 * i;
                        A1 = Gl + BCR_F + i, B1 = Gl + BCR_F + j, A2 = Gr + BCR_GM + i, B2 = Gr + BCR_GM + j, dst = lane;
                    } else
                        coupling(lane - 36);
                } else if (r == 1) {
                    if (lane < 8)
                        coupling(28 + lane);
                    else if (lane < 14)
                        rhs(lane - 8, 0, true);
                    else if (lane < 50)
                        rhs((lane - 14) / 6, 1 + (lane - 14) % 6, cols & 1);
                } else if (lane < 36)
                    rhs(lane / 6, 7 + lane % 6, true);
                double acc1 = 0., acc2 = 0.;
#pragma unroll
                for (int u = 0; u < 6; u++) {
                    acc1 = fma(A1[6 * u], B1[u * st], acc1);
                    acc2 = fma(A2[6 * u], B2[u * st], acc2);
                }
                if (dst >= 0) {
                    const double base = keep ? P[dst] : 0.;
                    P[dst] = (base - (use1 ? acc1 : 0.)) - (use2 ? acc2 : 0.);
                }
            }
            if (cols && lane == 0)
                s_cols[p - 1] = (unsigned char)cols;
        }
        lds_barrier();
        PGSTAMP(73 + 2 * levels);
    }
    return true;
    };
    if (!forward())
        return;
    // ---- substitution, the levels upwards: X_q = L^-T (GB_q - G-_q X_{q-s} - G+_q X_{q+s}), 6 x 13 ----
    for (int lev = levels - 1; lev >= 0; lev--) {
        const int s = 1 << lev, cnt = (n / s + 1) / 2;
        for (int t = wave; t < cnt; t += BCR_WAVES) {
            const int q = s * (2 * t + 1), b = a + q - 1;
            double *Q = sm + (q - 1) * BCR_ROW;
            const bool hl = q > s, hr = q + s <= n;
            const double *Xl = sm + ((hl ? q - s : q) - 1) * BCR_ROW + BCR_B;
            const double *Xr = sm + ((hr ? q + s : q) - 1) * BCR_ROW + BCR_B;
            double v[2];
#pragma unroll
            for (int k2 = 0; k2 < 2; k2++) {
                const int e = lane + 64 * k2;
                double acc = 0.;
                if (e < 78) {
                    const int i = e / 13, c = e - 13 * i;
                    acc = Q[BCR_B + e];
                    if (hl) {
#pragma unroll
                        for (int u = 0; u < 6; u++)
                            acc = fma(-Q[BCR_GM + 6 * i + u], Xl[13 * u + c], acc);
                    }
                    if (hr) {
#pragma unroll
                        for (int u = 0; u < 6; u++)
                            acc = fma(-Q[BCR_F + 6 * i + u], Xr[13 * u + c], acc);
                    }
                }
                v[k2] = acc;
            }
#pragma unroll
            for (int k2 = 0; k2 < 2; k2++)
                if (lane + 64 * k2 < 78)
                    Q[BCR_B + lane + 64 * k2] = v[k2];  // a lane's own entries
            svo::wave_lds_fence();
#pragma unroll
            for (int k2 = 0; k2 < 2; k2++) {
                const int e = lane + 64 * k2;
                double acc = 0.;
                if (e < 78) {
                    const int i = e / 13, c = e - 13 * i;
#pragma unroll
                    for (int u = 0; u < 6; u++)
                        acc = fma(Q[6 * u + i], Q[BCR_B + 13 * u + c], acc);  // L^-T: Linv[u][i], zero for u < i
                }
                v[k2] = acc;
            }
            svo::wave_lds_fence();
#pragma unroll
            for (int k2 = 0; k2 < 2; k2++) {
                const int e = lane + 64 * k2;
                if (e < 78) {
                    const int i = e / 13, c = e - 13 * i;
                    Q[BCR_B + e] = v[k2];
                    if (c == 0)
                        Y[(size_t)b * 6 + i] = v[k2];
                    else if (c < 7)
                        Wl[(size_t)b * 36 + 6 * i + (c - 1)] = v[k2];
                    else
                        Wr[(size_t)b * 36 + 6 * i + (c - 7)] = v[k2];
                }
            }
        }
        lds_barrier();
        PGSTAMP(90 + lev);
    }
    // ---- the closures that end inside this segment: six columns each, two closures to a pass through the factor ----
    for (int cc = ch.cptr[blockIdx.x]; cc < ch.cptr[blockIdx.x + 1]; cc += 2) {
        const bool two = cc + 1 < ch.cptr[blockIdx.x + 1];
        const int jr[2] = {ch.lrow[cc], two ? ch.lrow[cc + 1] : -1}, trs[2] = {ch.tr[cc], two ? ch.tr[cc + 1] : 0};
        const double *Hs[2] = {eo + (size_t)ch.edge[cc] * EO_FIELDS + EO_HIJ,
                               eo + (size_t)ch.edge[two ? cc + 1 : cc] * EO_FIELDS + EO_HIJ};
        double *wouts[2] = {Wc + (size_t)ch.wbase[cc] * 36, Wc + (size_t)ch.wbase[two ? cc + 1 : cc] * 36};
        for (int e = tid; e < n * 78; e += NT) {  // B = E_j H[j][i]: the first closure in the columns 1 .. 6, the second in 7 .. 12
            const int p = e / 78, k = e - 78 * p, r = k / 13, c = k - 13 * r;
            double v = 0.;
            if (c >= 1) {
                const int g2 = c >= 7 ? 1 : 0, cl = c - (g2 ? 7 : 1);
                if (p == jr[g2])
                    v = trs[g2] ? Hs[g2][6 * cl + r] : Hs[g2][6 * r + cl];
            }
            sm[p * BCR_ROW + BCR_B + k] = v;
        }
        lds_barrier();
        // Down: a closure's columns live in ONE row that is eliminated per level (the endpoint itself at its own level,
        // then whichever of the two rows it was folded into goes next), so a wave walks them up the elimination tree on its
        // own -- wave 0 the first closure's columns, wave 1 the second's -- with no workgroup barrier; the same operations
        // in the same order as the general sweep would do for these columns.  (The general sweep -- every wave through every
        // level with two barriers each, nearly all of them idle -- was 12 of a pass's 27 us.)
        if (wave < (two ? 2 : 1)) {
            const int c0 = wave ? 7 : 1;
            int flagged[4], nf = 1;
            flagged[0] = jr[wave] + 1;  // 1-based rows that carry the columns and have not been eliminated
            for (int s = 1; s <= n; s <<= 1) {
                int q = 0;
                for (int f = 0; f < nf; f++)
                    if ((flagged[f] & (2 * s - 1)) == s)
                        q = flagged[f];  // the one eliminated at this level (at most one: see above)
                if (!q)
                    continue;
                double *Q = sm + (q - 1) * BCR_ROW;
                const int i = lane / 6, c = c0 + lane % 6;
                double acc = 0.;
                if (lane < 36) {  // GB = Linv B, these six columns
#pragma unroll
                    for (int u = 0; u < 6; u++)
                        acc = fma(Q[6 * i + u], Q[BCR_B + 13 * u + c], acc);
                }
                svo::wave_lds_fence();
                if (lane < 36)
                    Q[BCR_B + 13 * i + c] = acc;
                svo::wave_lds_fence();
                int keep = 0;
                for (int f = 0; f < nf; f++)
                    if (flagged[f] != q)
                        flagged[keep++] = flagged[f];
                nf = keep;
                for (int side = 0; side < 2; side++) {  // into q - s through G-, into q + s through G+
                    const int p = side ? q + s : q - s;
                    if (p < 1 || p > n)
                        continue;
                    double *P = sm + (p - 1) * BCR_ROW;
                    const double *G = Q + (side ? BCR_F : BCR_GM);
                    if (lane < 36) {
                        double a2 = 0.;
#pragma unroll
                        for (int u = 0; u < 6; u++)
                            a2 = fma(G[6 * u + i], Q[BCR_B + 13 * u + c], a2);
                        P[BCR_B + 13 * i + c] -= a2;
                    }
                    bool known = false;
                    for (int f = 0; f < nf; f++)
                        known |= flagged[f] == p;
                    if (!known && nf < 4)
                        flagged[nf++] = p;
                }
                svo::wave_lds_fence();
            }
        }
        lds_barrier();
        const int ncols = two ? 72 : 36;
        for (int lev = levels - 1; lev >= 0; lev--) {
            const int s = 1 << lev, cnt = (n / s + 1) / 2;
            for (int t = wave; t < cnt; t += BCR_WAVES) {
                const int q = s * (2 * t + 1);
                double *Q = sm + (q - 1) * BCR_ROW;
                const bool hl = q > s, hr = q + s <= n;
                const double *Xl = sm + ((hl ? q - s : q) - 1) * BCR_ROW + BCR_B;
                const double *Xr = sm + ((hr ? q + s : q) - 1) * BCR_ROW + BCR_B;
                double v[2];
                int ii[2], cs2[2];
#pragma unroll
                for (int k2 = 0; k2 < 2; k2++) {  // entry e: the first closure's 36, then the second's
                    const int e = lane + 64 * k2, g2 = e >= 36 ? 1 : 0, el = e - 36 * g2;
                    const int i = el / 6, c = (g2 ? 7 : 1) + el % 6;
                    ii[k2] = i, cs2[k2] = c;
                    double acc = 0.;
                    if (e < ncols) {
                        acc = Q[BCR_B + 13 * i + c];
                        if (hl) {
#pragma unroll
                            for (int u = 0; u < 6; u++)
                                acc = fma(-Q[BCR_GM + 6 * i + u], Xl[13 * u + c], acc);
                        }
                        if (hr) {
#pragma unroll
                            for (int u = 0; u < 6; u++)
                                acc = fma(-Q[BCR_F + 6 * i + u], Xr[13 * u + c], acc);
                        }
                        Q[BCR_B + 13 * i + c] = acc;  // a lane's own entry
                    }
                    v[k2] = acc;
                }
                svo::wave_lds_fence();
#pragma unroll
                for (int k2 = 0; k2 < 2; k2++) {
                    double acc = 0.;
                    if (lane + 64 * k2 < ncols) {
#pragma unroll
                        for (int u = 0; u < 6; u++)
                            acc = fma(Q[6 * u + ii[k2]], Q[BCR_B + 13 * u + cs2[k2]], acc);
                    }
                    v[k2] = acc;
                }
                svo::wave_lds_fence();
#pragma unroll
                for (int k2 = 0; k2 < 2; k2++) {
                    const int e = lane + 64 * k2;
                    if (e < ncols) {
                        Q[BCR_B + 13 * ii[k2] + cs2[k2]] = v[k2];
                        const int g2 = e >= 36 ? 1 : 0;
                        wouts[g2][(size_t)(q - 1) * 36 + 6 * ii[k2] + (cs2[k2] - (g2 ? 7 : 1))] = v[k2];
                    }
                }
            }
            lds_barrier();
        }
    }
}

// Reduced (separator) system, assembled by gathers.  Block k of the launch owns one nonzero
// 6x6 block (rb_row >= rb_col, in separator indices) or, for k >= n_blocks, the right-hand side
// of separator k - n_blocks.  Sources src[ptr[k] .. ptr[k+1]) = (kind, idx) are added in list order; the kinds, and those of a
// term's A and W, are the enums of pg_solve_plan.hip.h, which builds the lists.
__global__ __launch_bounds__(64) void pg_reduce_kernel(int n_blocks, int m, const int *__restrict__ rb_row,
                                                       const int *__restrict__ rb_col, const int *__restrict__ ptr,
                                                       const int2 *__restrict__ src, const PgTerm *__restrict__ terms,
                                                       const double *__restrict__ Dg, const double *__restrict__ Cc,
                                                       const double *__restrict__ rneg, const double *__restrict__ eo,
                                                       const double *__restrict__ Y, const double *__restrict__ Wl,
                                                       const double *__restrict__ Wr, const double *__restrict__ Wc,
                                                       double *__restrict__ R, int ldr, double *__restrict__ rR)
{
    const int k = blockIdx.x, lane = threadIdx.x;
    // A^T[p][t] = H[t][p] of a term = base[sa * t + sb * p]; the kinds below A_HIJ read Cc, the odd ones are the transposes
    auto a_of = [&](const PgTerm &tm, const double *&base, int &sa, int &sb) {
        base = tm.a_kind < psp::A_HIJ ? Cc + (size_t)tm.a * 36 : eo + (size_t)tm.a * EO_FIELDS + EO_HIJ;
        sa = (tm.a_kind & 1) ? 1 : 6;
        sb = (tm.a_kind & 1) ? 6 : 1;
    };
    if (k < n_blocks) {
        if (lane >= 36)
            return;
        const int p = lane / 6, q = lane - 6 * p;
        double acc = 0;
        for (int t = ptr[k]; t < ptr[k + 1]; t++) {
            const int kind = src[t].x, idx = src[t].y;
            double v = 0;
            switch (kind) {
            case psp::SRC_DG: v = Dg[(size_t)idx * 36 + lane]; break;
            case psp::SRC_CC: v = Cc[(size_t)idx * 36 + lane]; break;
            case psp::SRC_HIJ: v = eo[(size_t)idx * EO_FIELDS + EO_HIJ + lane]; break;
            case psp::SRC_HIJ_T: v = eo[(size_t)idx * EO_FIELDS + EO_HIJ + 6 * q + p]; break;
            default: {  // SRC_TERM
                const PgTerm tm = terms[idx];
                const double *W = (tm.w_kind == psp::W_L ? Wl : tm.w_kind == psp::W_R ? Wr : Wc) + (size_t)tm.w * 36, *A;
                int sa, sb;
                a_of(tm, A, sa, sb);
                for (int t2 = 0; t2 < 6; t2++)
                    v -= A[sa * t2 + sb * p] * W[6 * t2 + q];
            }
            }
            acc += v;
        }
        R[(size_t)(6 * rb_row[k] + p) * ldr + 6 * rb_col[k] + q] = acc;
    } else {
        if (lane >= 6)
            return;
        const int sidx = k - n_blocks;
        if (sidx >= m)
            return;
        const int kk = n_blocks + sidx;
        double acc = 0;
        for (int t = ptr[kk]; t < ptr[kk + 1]; t++) {
            const int kind = src[t].x, idx = src[t].y;
            double v = 0;
            if (kind == psp::SRC_DG)
                v = rneg[(size_t)idx * 6 + lane];
            else {  // SRC_TERM, W_Y
                const PgTerm tm = terms[idx];
                const double *A;
                int sa, sb;
                a_of(tm, A, sa, sb);
                for (int t2 = 0; t2 < 6; t2++)
                    v -= A[sa * t2 + sb * lane] * Y[(size_t)tm.w * 6 + t2];
            }
            acc += v;
        }
        rR[6 * sidx + lane] = acc;
    }
}

// ---- blocked dense Cholesky of the reduced system (lower triangle, row-major, ld = ldr) ------
// Tile step kb:  every trailing tile (i, j), kb < j <= i:  A_ij -= P_i P_j^T with P_i = A_i,kb Tinv_kb^T (the tile
//                (i, kb+1) also stores P_i as the factor's block (i, kb));
//                the workgroup of the tile (kb+1, kb+1) goes on to factorise it in LDS -- the next step's diagonal tile --
//                and leaves the inverse of its factor in Tinv[kb+1] (the factor itself is not needed again).
// ONE launch per tile step (round 3 had two: the critical path of a step was the diagonal tile's update followed, across a
// launch boundary and a round trip through HBM, by its factorisation).  The first tile has a launch of its own.
// Column kb of A is only read in step kb, the factor goes to a separate array: no races.

// Cholesky of the 48 x 48 tile in sL (lower triangle; what is above the diagonal is never read) and the inverse of the
// factor into sX (zeroed here), blocked by 6 inside the tile.  The serial chain is the eight 6 x 6 diagonal blocks'
// FACTORS (wave_chol6_regs, by wave 0); everything else is arranged around it, two barriers per block step:
//   P  the panel below the diagonal block, L21 L11^T = A21, and the inverse's block row, L11 X[b][c] = -Z[b][c] (Z =
//      sum_{c <= k < b} L[b][k] X[k][c] has been accumulated in place): forward substitutions with L11 and the pivots'
//      reciprocals, a thread per row / per column -- and wave 0 forms L11^-1 meanwhile (nobody waits for it: it is the
//      inverse's diagonal block, read in Q);
//   Q  wave 0 takes the NEXT diagonal block's update out of the panel and factorises it, while waves 1..3 do the trailing
//      update A22 -= L21 L21^T and add this step's terms to Z in the rows below -- 3 x 3 blocks per thread on a 16 x 16
//      thread grid, the same code for both (the rows of wave 0's threads are done with by then).
// (Round 3: factor, panel, trailing update one after the other with three barriers, then the inverse from inverted
// halves -- 26 us a tile; 10.6 us with the 6 x 6 inverse still in wave 0's chain.)
// sL6: L11 (zeros above the diagonal), sR6: the six reciprocals.  Returns (to every thread) 0 or 1 + the row of the first
// non-positive pivot.
__device__ __forceinline__ int pg_potf2_lds(bool dbg, double *sL, double *sX, double *sS6, double *sL6, double *sR6,
                                            int *s_bad, int tid)
{
    constexpr int LD = TB + 1, NB6 = TB / 6;
    const int tr = tid >> 4, tc = tid & 15;
    for (int e = tid; e < TB * LD; e += 256)
        sX[e] = 0.;
    if (tid == 0)
        *s_bad = 0;
    lds_barrier();
    double fa[6], fr[6];  // wave 0: the current diagonal block's factor, kept for its inverse
    // the diagonal block at o2, with the update from the panel columns o .. o+5 (o < 0: none), by wave 0
    auto diag_block = [&](int o, int o2) {
        if (tid < 36) {
            const int i = tid / 6, j = tid - 6 * i, hi = o2 + (i > j ? i : j), lo = o2 + (i > j ? j : i);
            double v = sL[hi * LD + lo];  // symmetric from the lower triangle
            if (o >= 0) {
#pragma unroll
                for (int t = 0; t < 6; t++)
                    v -= sL[hi * LD + o + t] * sL[lo * LD + o + t];
            }
            sS6[tid] = v;
        }
        svo::wave_lds_fence();
        if (!wave_chol6_regs(sS6, tid, fa, fr) && tid == 0 && *s_bad == 0)
            *s_bad = 1 + o2;
        if (tid < 6) {
#pragma unroll
            for (int c = 0; c < 6; c++) {
                const double v = c <= tid ? fa[c] : 0.;  // zero above the diagonal
                sL6[6 * tid + c] = v;
                sL[(o2 + tid) * LD + o2 + c] = v;
            }
            sR6[tid] = fr[tid];
        }
    };
    if (tid < 64)
        diag_block(-1, 0);
    lds_barrier();
    for (int blk = 0; blk < NB6; blk++) {
        const int o = 6 * blk, below = TB - o - 6;
        PGSTAMP(2 + 2 * blk);
        // ---- P ----
        if (tid < 64) {  // L11^-1, the inverse's diagonal block
            double x[6];
            wave_inv6_regs(fa, fr, tid, x);
            if (tid < 6) {
#pragma unroll
                for (int r = 0; r < 6; r++)
                    sX[(o + r) * LD + o + tid] = x[r];
            }
        } else if (tid - 64 < o) {  // column tid - 64 of the inverse's block row: L11 x = -z, in place
            double *col = sX + o * LD + (tid - 64);
            double x[6];
#pragma unroll
            for (int i = 0; i < 6; i++) {
                double acc = -col[i * LD];
#pragma unroll
                for (int t = 0; t < i; t++)
                    acc -= sL6[6 * i + t] * x[t];
                x[i] = acc * sR6[i];
            }
#pragma unroll
            for (int i = 0; i < 6; i++)
                col[i * LD] = x[i];
        } else if (tid >= 128 && tid - 128 < below) {  // row o + 6 + (tid - 128) of the panel: x L11^T = a
            double *row = sL + (o + 6 + tid - 128) * LD + o;
            double x[6];
#pragma unroll
            for (int c = 0; c < 6; c++) {
                double acc = row[c];
#pragma unroll
                for (int t = 0; t < c; t++)
                    acc -= x[t] * sL6[6 * c + t];
                x[c] = acc * sR6[c];
            }
#pragma unroll
            for (int c = 0; c < 6; c++)
                row[c] = x[c];
        }
        lds_barrier();
        PGSTAMP(3 + 2 * blk);
        if (blk == NB6 - 1)
            break;
        // ---- Q ----
        const int o2 = o + 6;
        if (tid < 64)
            diag_block(o, o2);
        else {
            // the 3 x 3 block (R, C) of this thread: out[a][b] (-/+)= sum_t sL[3R+a][o+t] * Y[b][t]
            //   3C >= o2: trailing update, Y[b][t] = sL[3C+b][o+t] (the next diagonal block is wave 0's);
            //   3C <  o2: Z of the rows below, Y[b][t] = sX[o+t][3C+b]
            int R = tr, C = tc;
            bool on = tc <= tr && 3 * tr >= o2;
            if (blk == 0 && tr == 4 && tc >= 5 && tc <= 8) {  // rows 6 .. 11 belong to wave 0's threads: their Z blocks
                R = 2 + ((tc - 5) >> 1);                      // (columns 0 .. 5) go to four threads that have nothing to do
                C = (tc - 5) & 1;
                on = true;
            }
            const bool trail = 3 * C >= o2;
            if (trail && 3 * R < o2 + 6)
                on = false;
            if (on) {
                const double *px = sL + (3 * R) * LD + o;
                const double *py = trail ? sL + (3 * C) * LD + o : sX + o * LD + 3 * C;
                const int sb = trail ? LD : 1, stt = trail ? 1 : LD;
                double acc[3][3] = {{0., 0., 0.}, {0., 0., 0.}, {0., 0., 0.}};
#pragma unroll
                for (int t = 0; t < 6; t++) {
                    const double x0 = px[t], x1 = px[LD + t], x2 = px[2 * LD + t];
                    const double y0 = py[t * stt], y1 = py[sb + t * stt], y2 = py[2 * sb + t * stt];
                    acc[0][0] = fma(x0, y0, acc[0][0]);
                    acc[0][1] = fma(x0, y1, acc[0][1]);
                    acc[0][2] = fma(x0, y2, acc[0][2]);
                    acc[1][0] = fma(x1, y0, acc[1][0]);
                    acc[1][1] = fma(x1, y1, acc[1][1]);
                    acc[1][2] = fma(x1, y2, acc[1][2]);
                    acc[2][0] = fma(x2, y0, acc[2][0]);
                    acc[2][1] = fma(x2, y1, acc[2][1]);
                    acc[2][2] = fma(x2, y2, acc[2][2]);
                }
                // (a diagonal block's entries above the diagonal are written too: nobody reads them)
                double *dst = (trail ? sL : sX) + (3 * R) * LD + 3 * C;
                const double sg = trail ? -1. : 1.;
#pragma unroll
                for (int a = 0; a < 3; a++)
#pragma unroll
                    for (int b2 = 0; b2 < 3; b2++)
                        dst[a * LD + b2] += sg * acc[a][b2];
            }
        }
        lds_barrier();
    }
    PGSTAMP(50);
    return *s_bad;
}

// The solve's layout of a 48 x 48 block M (a factor block below the diagonal, or a diagonal tile's inverse): it applies
// M^T to a vector with thread (r, part) of 48 x 8 taking the rows part, part + 8, ... of column r, so entry (row, col) lives
// at col * 48 + (row % 8) * 6 + row / 8 -- a thread's six entries are 48 contiguous bytes, a wave's 3 KB.
__device__ __forceinline__ int pg_solve_slot(int row, int col) { return col * TB + (row & 7) * 6 + (row >> 3); }

// a diagonal tile's inverse, from LDS to its two arrays: row-major for the next step's products, the solve's layout
__device__ __forceinline__ void pg_store_factor_tile(const double *sX, double *__restrict__ Tinv, double *__restrict__ Tp,
                                                     int kb, int tid)
{
    constexpr int LD = TB + 1;
    for (int e = tid; e < TB * TB; e += 256) {
        const int r = e / TB, c = e - TB * r;
        Tinv[(size_t)kb * TB * TB + e] = c <= r ? sX[r * LD + c] : 0.;
    }
    for (int d = tid; d < TB * TB; d += 256) {  // destination order: coalesced stores
        const int c = d / TB, w = d - TB * c, r = (w / 6) + 8 * (w % 6);
        Tp[(size_t)kb * TB * TB + d] = c <= r ? sX[r * LD + c] : 0.;
    }
}

// the first diagonal tile (nothing to update before it)
__global__ __launch_bounds__(256) void pg_dense_potf2_kernel(const double *__restrict__ A, double *__restrict__ Tinv,
                                                             double *__restrict__ Tp, int ldr, int kb,
                                                             int *__restrict__ status, int status_base)
{
    constexpr int LD = TB + 1;
    __shared__ double sL[TB * LD], sX[TB * LD];
    __shared__ double sS6[36], sL6[36], sR6[6];
    __shared__ int s_bad;
    const int tid = threadIdx.x;
    for (int e = tid; e < TB * TB; e += 256) {
        const int r = e / TB, c = e - TB * r;
        sL[r * LD + c] = c <= r ? A[(size_t)(kb * TB + r) * ldr + kb * TB + c] : 0.;
    }
    const bool dbg = true;
    PGSTAMP(0);
    __syncthreads();
    PGSTAMP(1);
    const int bad = pg_potf2_lds(true, sL, sX, sS6, sL6, sR6, &s_bad, tid);
    if (bad && tid == 0)
        atomicMax(status, status_base + kb * TB + bad);  // keep going with whatever is there: the host reports the failure
    pg_store_factor_tile(sX, Tinv, Tp, kb, tid);
    __syncthreads();
    PGSTAMP(51);
}

// C = X Y^T for 48 x 48 tiles in LDS on the matrix cores (v_mfma_f64_16x16x4_f64): waves 0..2 take a block row of three
// 16 x 16 blocks each, twelve k-steps of four.  Lane l feeds A[i = l & 15][k = l >> 4] = X[16 I + i][4 s + k] and
// B[k][j = l & 15] = Y[16 J + j][4 s + k], and holds D[row = (l >> 4) + 4 reg][col = l & 15] in its four results.  f64 MFMA
// has the rate of the vector unit on this chip; what it buys is LDS traffic: two reads per 1024 multiply-adds instead of
// six per nine (3 x 3 register blocks per thread on the vector unit were LDS-bound at 2.4 us a product; 1.0 us now).
// TRI: Y is lower triangular (block column J needs k < 16 (J + 1) only).  LOWER: only the blocks J <= I are stored.
// sC may be sX: a wave reads only its own 16 rows of X and writes only those rows of C.
typedef double pg_double4 __attribute__((ext_vector_type(4)));
template <bool TRI, bool LOWER>
__device__ __forceinline__ void pg_tile_mult_mfma(const double *sX, const double *sY, double *sC, int tid)
{
    constexpr int LD = TB + 1;
    const int I = tid >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4;
    if (I >= 3)
        return;
    const double *px = sX + (16 * I + li) * LD + lk, *py = sY + li * LD + lk;
    pg_double4 acc[3];
#pragma unroll
    for (int J = 0; J < 3; J++)
        acc[J] = (pg_double4){0., 0., 0., 0.};
#pragma unroll
    for (int s4 = 0; s4 < TB / 4; s4++) {
        const double a = px[4 * s4];
#pragma unroll
        for (int J = 0; J < 3; J++) {
            if (TRI && s4 >= 4 * (J + 1))
                continue;
            const double b = py[16 * J * LD + 4 * s4];
            acc[J] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[J], 0, 0, 0);
        }
    }
#pragma unroll
    for (int J = 0; J < 3; J++) {
        if (LOWER && J > I)
            continue;
#pragma unroll
        for (int reg = 0; reg < 4; reg++)
            sC[(16 * I + lk + 4 * reg) * LD + 16 * J + li] = acc[J][reg];
    }
}

// The forward substitution of the solve rides along: the workgroup of a diagonal tile (j, j) has the factor's block
// L_j,kb = P_j at hand, forms y_kb = Tinv_kb b_kb (48 x 48, every such workgroup for itself) and takes L_j,kb y_kb off
// b_j; the first of them leaves y_kb in `yout`.  The solve kernel is left with the last tile's y and the backward sweep.
// Workgroup 0 owns the tile (kb+1, kb+1): it keeps the updated tile in LDS and factorises it (see above).
__global__ __launch_bounds__(256) void pg_dense_step_kernel(double *__restrict__ A, double *__restrict__ Ls,
                                                            double *__restrict__ Tinv, double *__restrict__ Tp, int ldr,
                                                            int T, int kb,
                                                            double *__restrict__ rhs, double *__restrict__ yout,
                                                            int *__restrict__ status, int status_base)
{
    __shared__ double sI[TB * (TB + 1)], sPi[TB * (TB + 1)], sPj[TB * (TB + 1)], sA[TB * (TB + 1)];
    __shared__ double s_y[TB], s_b[TB];
    __shared__ double sS6[36], sL6[36], sR6[6];
    __shared__ int s_bad;
    constexpr int LD = TB + 1;
    const int tid = threadIdx.x, tr = tid >> 4, tc = tid & 15;
    // linear tile index -> (i, j) with kb < j <= i < T.  The LAST workgroup of the launch is workgroup 0's stand-in for the
    // right-hand side of block row kb+1 (it forms P_kb+1 once more and leaves): workgroup 0 is the launch's critical path.
    const bool rhs_only = blockIdx.x == gridDim.x - 1;
    int t = rhs_only ? 0 : blockIdx.x, i = kb + 1;
    while (t >= i - kb) {
        t -= i - kb;
        i++;
    }
    const int j = kb + 1 + t;
    const bool diag = i == j, keep = !(diag && tc > tr);  // a diagonal tile: whole 3 x 3 blocks above it are skipped
    const bool dbg = blockIdx.x == 0 && kb == 0;
    PGSTAMP(60);
    // the tile this workgroup updates: asked for now, used at the end
    double old[3][3];
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b2 = 0; b2 < 3; b2++)
            old[a][b2] = keep ? A[(size_t)(i * TB + 3 * tr + a) * ldr + j * TB + 3 * tc + b2] : 0.;
    {  // Tinv_kb, A_i,kb, A_j,kb: every load on its way before the first is waited for
        double vI[9], vA[9], vJ[9];
#pragma unroll
        for (int q = 0; q < 9; q++) {
            const int e = tid + 256 * q, r = e / TB, c = e - TB * r;
            vI[q] = Tinv[(size_t)kb * TB * TB + e];
            vA[q] = A[(size_t)(i * TB + r) * ldr + kb * TB + c];
            vJ[q] = diag ? 0. : A[(size_t)(j * TB + r) * ldr + kb * TB + c];
        }
#pragma unroll
        for (int q = 0; q < 9; q++) {
            const int e = tid + 256 * q, r = e / TB, c = e - TB * r;
            sI[r * LD + c] = c <= r ? vI[q] : 0.;  // lower triangular
            sA[r * LD + c] = vA[q];
            if (!diag)
                sPj[r * LD + c] = vJ[q];  // A_j,kb for now
        }
    }
    if (diag && tid < TB)
        s_b[tid] = rhs[kb * TB + tid];
    __syncthreads();
    PGSTAMP(61);
    pg_tile_mult_mfma<true, false>(sA, sI, sPi, tid);  // P_i = A_i,kb * Tinv^T
    if (!diag)
        pg_tile_mult_mfma<true, false>(sPj, sI, sPj, tid);  // P_j = A_j,kb * Tinv^T, in place
    __syncthreads();
    if (diag && blockIdx.x != 0) {  // the right-hand side of block row j (see above); sI is the lower-triangular Tinv_kb; four lanes per row
        const int rr = tid >> 2, part = tid & 3;
        if (tid < 4 * TB) {
            double a = 0;
#pragma unroll 4
            for (int c = part; c < TB; c += 4)  // (zeros above the diagonal)
                a += sI[rr * LD + c] * s_b[c];
            a += __shfl_xor(a, 1, 64);
            a += __shfl_xor(a, 2, 64);
            if (part == 0) {
                s_y[rr] = a;
                if (rhs_only)
                    yout[kb * TB + rr] = a;
            }
        }
        __syncthreads();
        if (tid < 4 * TB) {
            double a = 0;
#pragma unroll 4
            for (int c = part; c < TB; c += 4)
                a += sPi[rr * LD + c] * s_y[c];
            a += __shfl_xor(a, 1, 64);
            a += __shfl_xor(a, 2, 64);
            if (part == 0)
                rhs[j * TB + rr] -= a;
        }
        if (rhs_only)
            return;
        __syncthreads();  // Tinv_kb in sI has been used: the product below goes there
    }
    PGSTAMP(62);
    if (diag)
        pg_tile_mult_mfma<false, true>(sPi, sPi, sI, tid);
    else
        pg_tile_mult_mfma<false, false>(sPi, sPj, sI, tid);
    __syncthreads();
    double acc[3][3];  // this thread's 3 x 3 block of P_i P_j^T
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b2 = 0; b2 < 3; b2++)
            acc[a][b2] = keep ? sI[(3 * tr + a) * LD + 3 * tc + b2] : 0.;
    PGSTAMP(63);
    if (j == kb + 1)  // the factor's block (i, kb), in the solve's layout
        for (int d = tid; d < TB * TB; d += 256) {
            const int c = d / TB, w = d - TB * c, r = (w / 6) + 8 * (w % 6);
            Ls[((size_t)i * T + kb) * TB * TB + d] = sPi[r * LD + c];
        }
    if (blockIdx.x != 0) {
        if (keep) {
#pragma unroll
            for (int a = 0; a < 3; a++)
#pragma unroll
                for (int b2 = 0; b2 < 3; b2++) {
                    const int r = 3 * tr + a, c = 3 * tc + b2;
                    if (diag && c > r)
                        continue;
                    A[(size_t)(i * TB + r) * ldr + j * TB + c] = old[a][b2] - acc[a][b2];
                }
        }
        return;
    }
    // workgroup 0: the tile (kb+1, kb+1) has had its last update -- it stays in LDS and is factorised here
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b2 = 0; b2 < 3; b2++)
            sA[(3 * tr + a) * LD + 3 * tc + b2] = keep ? old[a][b2] - acc[a][b2] : 0.;
    __syncthreads();  // also: sI, sPj and the right-hand side's use of sPi are over
    PGSTAMP(64);
    const int bad = pg_potf2_lds(false, sA, sPj, sS6, sL6, sR6, &s_bad, tid);
    if (bad && tid == 0)
        atomicMax(status, status_base + (kb + 1) * TB + bad);
    PGSTAMP(65);
    pg_store_factor_tile(sPj, Tinv, Tp, kb + 1, tid);
    __syncthreads();
    PGSTAMP(66);
}

// L^T x = y with the tiles' inverses (the forward substitution came with the factorisation, except for the last tile).
// One workgroup of 384 threads = 48 columns x 8 row parts; the vector and the running sums  acc_kb = sum_{i > kb}
// L_i,kb^T x_i  live in LDS.  Tile step i: x_i = Tinv_i^T (y_i - acc_i), then x_i's terms go onto the acc of every tile
// above.  The tile (i, i-1) and Tinv_{i-1}, which the next step waits for, are asked for one step ahead; this step's other
// blocks at the top of the step, two LDS-only barriers before they are used.  What made this kernel fast was the LAYOUT of
// the factor: with row-major blocks a thread's six values were six rows apart and a wave's load touched eight 64-byte
// pieces -- one compute unit got 16 GB/s out of it, 60 us for the megabyte of an 81-separator factor whatever the order
// of the loads (round 3: 94 us with a dependent load per row); in the solve's own layout (pg_solve_slot) the same data
// are three 16-byte loads per thread and 3 KB contiguous per wave: 25 us.
constexpr int PG_SOLVE_THREADS = TB * 8;
__device__ __forceinline__ double pg_sum8(double v)
{
    v = v + __shfl_xor(v, 1, 64);
    v = v + __shfl_xor(v, 2, 64);
    v = v + __shfl_xor(v, 4, 64);
    return v;
}
__global__ __launch_bounds__(PG_SOLVE_THREADS) void pg_dense_solve_kernel(const double *__restrict__ Ls,
                                                                          const double *__restrict__ Tinv,
                                                                          const double *__restrict__ Tp, int ldr, int T,
                                                                          const double *__restrict__ rhs, double *x)
{
    extern __shared__ double sv[];  // ldr entries (y, then x) + ldr (acc) + TB
    double *sacc = sv + ldr, *st = sacc + ldr;
    const int tid = threadIdx.x;
    const int r = tid >> 3, part = tid & 7;
#ifdef PG_STAMPS
    if (tid == 0)
        pg_dbg[99] = wall_clock64();
#endif
    // thread (r, part): the rows part, part + 8, ... of column r of a block -- six contiguous doubles in the solve's layout,
    // at a wave-uniform block base (scalar registers) + ONE per-thread offset for all blocks
    const int toff = r * TB + part * 6;
    auto load_block = [&](const double *base, double (&l)[6]) {
        const double2 *p2 = reinterpret_cast<const double2 *>(base + toff);
        const double2 v0 = p2[0], v1 = p2[1], v2 = p2[2];
        l[0] = v0.x, l[1] = v0.y, l[2] = v1.x, l[3] = v1.y, l[4] = v2.x, l[5] = v2.y;
    };
    auto load_tile = [&](int i, int kb, double (&l)[6]) { load_block(Ls + ((size_t)i * T + kb) * TB * TB, l); };
    auto load_tinv_t = [&](int kb, double (&l)[6]) { load_block(Tp + (size_t)kb * TB * TB, l); };
    double nti[6], ntile[6];
    load_tinv_t(T - 1, nti);
    load_tile(T - 1, T > 1 ? T - 2 : 0, ntile);
    // forward: y of the tiles 0 .. T-2 came with the factorisation (pg_dense_step_kernel left them in x, and took their
    // terms off the later blocks of rhs); the last tile's y = Tinv (its block of rhs) here
    for (int e = tid; e < ldr; e += PG_SOLVE_THREADS) {
        sv[e] = e < (T - 1) * TB ? x[e] : rhs[e];
        sacc[e] = 0.;
    }
    lds_barrier();
    {
        const int kb = T - 1;
        if (part == 0)
            st[r] = sv[kb * TB + r];
        lds_barrier();
        double a2 = 0;
        const double *ti = Tinv + (size_t)kb * TB * TB + r * TB;
        for (int c = part; c <= r; c += 8)
            a2 += ti[c] * st[c];
        a2 = pg_sum8(a2);
        lds_barrier();
        if (part == 0)
            sv[kb * TB + r] = a2;
    }
    const bool dbg = true;
    PGSTAMP(100);
    for (int i = T - 1; i >= 0; i--) {  // backward: x_i = Tinv_i^T (y_i - acc_i)
        PGSTAMP(101 + 2 * (i < 12 ? i : 12));
        double ti[6], tile[6], far[8][6];
#pragma unroll
        for (int q = 0; q < 6; q++) {
            // what was asked for a step ago is waited for HERE, with nothing else on its way (left to itself the compiler
            // finds the wait a few instructions after this step's loads have been issued, and waits for those as well)
            asm volatile("" : "+v"(nti[q]), "+v"(ntile[q]));
            ti[q] = nti[q];
            tile[q] = ntile[q];
        }
        // asked for now, used after x_i is known (two barriers further down): this step's tiles further up the column,
        // and what the next step waits for
        // (every load unconditional, on a clamped tile index: a load under a branch makes the compiler wait for all
        // loads at the join, and the point of issuing them here is that nobody waits)
#pragma unroll
        for (int u = 0; u < 8; u++)
            if (i - 2 - u >= 0)  // (wave-uniform)
                load_tile(i, i - 2 - u, far[u]);
        load_tinv_t(i > 0 ? i - 1 : 0, nti);
        load_tile(i > 0 ? i - 1 : 0, i > 1 ? i - 2 : 0, ntile);
        if (part == 0)
            st[r] = sv[i * TB + r] - sacc[i * TB + r];  // (r, part 0) is the only writer of sacc's column r
        lds_barrier();
        double a2 = 0;
#pragma unroll
        for (int q = 0; q < 6; q++)
            a2 += ti[q] * st[part + 8 * q];  // (zeros above the diagonal)
        a2 = pg_sum8(a2);
        if (part == 0)
            sv[i * TB + r] = a2;
        lds_barrier();
        PGSTAMP(102 + 2 * (i < 12 ? i : 12));
        const double *xi = sv + i * TB + part;
        auto onto_acc = [&](int kb, const double (&l)[6]) {  // acc_kb += L_i,kb^T x_i
            double a = 0;
#pragma unroll
            for (int q = 0; q < 6; q++)
                a += l[q] * xi[8 * q];
            a = pg_sum8(a);
            if (part == 0)
                sacc[kb * TB + r] += a;
        };
        if (i > 0)
            onto_acc(i - 1, tile);
#pragma unroll
        for (int u = 0; u < 8; u++)
            if (i - 2 - u >= 0)
                onto_acc(i - 2 - u, far[u]);
        for (int kb0 = i - 10; kb0 >= 0; kb0 -= 4) {  // a system of more than ten tiles: the rest, four at a time in flight
            double tl[4][6];
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (kb0 - u >= 0)
                    load_tile(i, kb0 - u, tl[u]);
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (kb0 - u >= 0)
                    onto_acc(kb0 - u, tl[u]);
        }
    }
    lds_barrier();
    PGSTAMP(127);
    for (int e = tid; e < ldr; e += PG_SOLVE_THREADS)
        x[e] = sv[e];
}

// dx of every block row -- separators copy their reduced solution, interior rows combine y - Wl x_l - Wr x_r (lsep /
// rsep: separator indices of the row's segment, -1 = none) -- and the vertex's update X <- X * fromVectorMQT(dx) in the
// same launch: six threads per row form dx, the first of them applies it.
constexpr int PG_UPD_ROWS = 32;
__global__ __launch_bounds__(PG_UPD_ROWS * 6) void pg_backsub_update_kernel(int nb, const int *__restrict__ sepidx,
                                                                            const int *__restrict__ lsep,
                                                                            const int *__restrict__ rsep,
                                                                            const double *__restrict__ xR,
                                                                            const double *__restrict__ Y,
                                                                            const double *__restrict__ Wl,
                                                                            const double *__restrict__ Wr,
                                                                            const int *__restrict__ rowseg,
                                                                            const int *__restrict__ seg_start,
                                                                            const int *__restrict__ cptr,
                                                                            const int *__restrict__ csep,
                                                                            const int *__restrict__ cwbase,
                                                                            const double *__restrict__ Wc,
                                                                            double *__restrict__ pose,
                                                                            const double *dx_add, double *dx_out)
{
    // iterative refinement (svo_pg_set_refinement): a first pass leaves its dx in dx_out and does not touch the poses; the
    // pass over the residual adds the first pass's dx (dx_add) and applies the sum.  With two or more passes the middle ones
    // accumulate in place, dx_add == dx_out (each thread reads its entry before it writes it): neither is __restrict__.
    __shared__ double s_dx[PG_UPD_ROWS * 6];
    const int t = blockIdx.x * (PG_UPD_ROWS * 6) + threadIdx.x;
    const int b = t / 6, r = t - 6 * b;
    if (b < nb) {
        const int si = sepidx[b];
        double v;
        if (si >= 0)
            v = xR[6 * si + r];
        else {
            v = Y[t];
            const int l = lsep[b], rr = rsep[b];
            if (l >= 0) {
#pragma unroll
                for (int c = 0; c < 6; c++)
                    v -= Wl[(size_t)b * 36 + 6 * r + c] * xR[6 * l + c];
            }
            if (rr >= 0) {
#pragma unroll
                for (int c = 0; c < 6; c++)
                    v -= Wr[(size_t)b * 36 + 6 * r + c] * xR[6 * rr + c];
            }
            const int sg = rowseg[b];  // the closures that end inside this row's segment
            for (int cc = cptr[sg]; cc < cptr[sg + 1]; cc++) {
                const double *W = Wc + (size_t)(cwbase[cc] + (b - seg_start[sg])) * 36 + 6 * r;
                const double *xs = xR + 6 * csep[cc];
#pragma unroll
                for (int c = 0; c < 6; c++)
                    v -= W[c] * xs[c];
            }
        }
        if (dx_add)
            v += dx_add[t];
        if (dx_out)
            dx_out[t] = v;
        s_dx[threadIdx.x] = v;
    }
    if (dx_out)
        return;
    __syncthreads();
    if (b >= nb || r != 0)
        return;
    const double *d = s_dx + threadIdx.x;
    const int v = b + 1;
    double D[7] = {d[0], d[1], d[2], 0, 0, 0, 1}, O[7];
    const double w = 1. - (d[3] * d[3] + d[4] * d[4] + d[5] * d[5]);
    if (w >= 0) {  // else: identity rotation (g2o fromCompactQuaternion)
        D[3] = d[3];
        D[4] = d[4];
        D[5] = d[5];
        D[6] = sqrt(w);
    }
    se3_mul(pose + 7 * v, D, O);
    q_normalize(O + 3);
    for (int k = 0; k < 7; k++)
        pose[7 * v + k] = O[k];
}

// Iterative refinement: r = rneg - H dx, every sum in double-double (error-free products through fma, two-sum
// accumulation), so that the residual of a solution that is good to 1e-6 still has ten correct digits.  Six threads per
// block row; a row's terms come from its incident edges' records in the assemble kernel's order.
__device__ __forceinline__ void dd_add_prod(double &hi, double &lo, double a, double b)
{
    const double p = a * b, e = fma(a, b, -p);
    const double s = hi + p, bb = s - hi;
    const double err = (hi - (s - bb)) + (p - bb);
    hi = s;
    lo += err + e;
}
__global__ __launch_bounds__(PG_UPD_ROWS * 6) void pg_residual_kernel(int nb, const int *__restrict__ incptr,
                                                                      const int *__restrict__ inc, const int *__restrict__ efrom,
                                                                      const int *__restrict__ eto, const double *__restrict__ eo,
                                                                      const double *__restrict__ rneg, const double *__restrict__ dx,
                                                                      double *__restrict__ r_out)
{
    const int t = blockIdx.x * (PG_UPD_ROWS * 6) + threadIdx.x;
    const int b = t / 6, p = t - 6 * b;
    if (b >= nb)
        return;
    const int v = b + 1;
    double hi = rneg[t], lo = 0.;
    for (int k = incptr[v]; k < incptr[v + 1]; k++) {
        const int e = inc[k] >> 1, role = inc[k] & 1;
        const double *o = eo + (size_t)e * EO_FIELDS;
        const int other = role ? efrom[e] : eto[e];
        // own block: H_vv' = Jv^T Jv (symmetric); the coupling: Ji^T Jj as stored for role 0 (v = i), its transpose for role 1
        const double *own = o + (role ? EO_HJJ : EO_HII);
        const double *dv = dx + 6 * (size_t)b;
#pragma unroll
        for (int q = 0; q < 6; q++)
            dd_add_prod(hi, lo, -own[6 * p + q], dv[q]);
        if (other >= 1) {
            const double *dw = dx + 6 * (size_t)(other - 1);
#pragma unroll
            for (int q = 0; q < 6; q++)
                dd_add_prod(hi, lo, -o[EO_HIJ + (role ? 6 * q + p : 6 * p + q)], dw[q]);
        }
    }
    r_out[t] = hi + lo;
}

}  // namespace

// DevBuf::ensure drops the old content; this one carries the first `keep` bytes over
static int ensure_keep(DevBuf &b, size_t bytes, size_t keep, hipStream_t st)
{
    if (bytes <= b.cap)
        return SVO_OK;
    if (keep == 0 || !b.p)
        return b.ensure(bytes);
    DevBuf nb;
    int rc = nb.ensure(bytes + bytes / 2);  // a graph grows vertex by vertex: leave room
    if (rc)
        return rc;
    if (hipMemcpyAsync(nb.p, b.p, keep, hipMemcpyDeviceToDevice, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) {
        nb.release();
        svo_set_error("pose graph: cannot carry the device copy over");
        return SVO_ERR_HIP;
    }
    b.release();
    b = nb;
    return SVO_OK;
}

struct svo_posegraph {
    svo_ctx *ctx = nullptr;
    std::vector<double> pose;  // 7 per vertex
    std::vector<int> efrom, eto;
    std::vector<double> meas;  // 7 per edge
    // Information matrices, lazily: EMPTY while every edge has the identity (no vector exists until a non-identity
    // matrix arrives, and the identity kernel runs); else 21 per edge (upper triangle, row-major) with has_info[e] == 0
    // and the identity's numbers for the edges that store none.  n_info: edges with has_info set.
    std::vector<double> info;
    std::vector<char> has_info;
    int n_info = 0;
    // Robust kernels, lazily like the information: EMPTY while no edge carries one (the two non-robust linearisations run); else a
    // kind and its parameter per edge.  n_robust: edges whose kind is not NONE.  lc_kind / lc_delta: what a new closure gets.
    std::vector<int> rkind;
    std::vector<double> rdelta;
    int n_robust = 0;
    int lc_kind = SVO_PG_ROBUST_NONE;
    double lc_delta = 0;
    // the edges of the last solve when its final linearisation was a robust one and nothing has changed since (EO_W of d_eo
    // holds the weights at the current estimates), else -1
    int eo_w_ne = -1;
    int prev = -1;
    // What the device already holds.  The graph only grows between two solves (augmentNode /
    // addLoopClosure append), and after a solve the device poses ARE the host poses, so the next
    // solve uploads the new vertices and edges only.  initializeGraph / read_g2o / a failed solve reset this.
    int dev_nv = 0, dev_ne = 0;
    // d_info follows the edges the way d_meas does: dev_ninfo edges' matrices are on the device (0: none, or changed
    // under an edge already uploaded -- the next weighted solve uploads all of them).  The elimination structure below
    // does not depend on the information and is not rebuilt for it.
    int dev_ninfo = 0;
    // The elimination structure (separators, segments, gather lists) of the graph as last built; reused
    // as long as no vertex or edge was added.  The host copies (the plan's vectors) stay alive here so that their uploads
    // need no synchronisation of their own.
    int built_nv = -1, built_ne = -1;
    pg_solve_plan::Plan plan;
    DevBuf d_rkind, d_rdelta, d_eval;
    DevBuf d_pose, d_from, d_to, d_meas, d_info, d_eo, d_incptr, d_inc, d_struct, d_Dg, d_Cc, d_rneg, d_Y,
        d_Wl, d_Wr, d_Wc, d_R, d_Lo, d_Tinv, d_rR, d_xR, d_misc, d_dx, d_res;
    int refine = 0;  // iterative-refinement passes per Gauss-Newton iteration (svo_pg_set_refinement)
    int nv() const { return (int)(pose.size() / 7); }
    int ne() const { return (int)efrom.size(); }
};

static void pg_drop_info(svo_posegraph *g)
{
    g->info.clear();
    g->has_info.clear();
    g->n_info = 0;
    g->dev_ninfo = 0;
}

// A usable information matrix is finite and positive definite (pg_g2o::check_info); `what` names the edge
static int pg_check_info(const double *info21, const char *what, int e)
{
    const std::string why = pg_g2o::check_info(info21, what, e);
    if (why.empty())
        return SVO_OK;
    svo_set_error("%s", why.c_str());
    return SVO_ERR_ARG;
}

// Stores the (checked) information of edge e; NULL or the exact identity = none.  The edge must exist.
static void pg_store_info(svo_posegraph *g, int e, const double *info21)
{
    const bool none = !info21 || !memcmp(info21, pg_g2o::INFO_IDENTITY, sizeof(pg_g2o::INFO_IDENTITY));
    if (g->info.empty()) {
        if (none)
            return;
        g->has_info.assign(g->ne(), 0);
        g->info.resize((size_t)21 * g->ne());
        for (int k = 0; k < g->ne(); k++)
            memcpy(&g->info[(size_t)21 * k], pg_g2o::INFO_IDENTITY, sizeof(pg_g2o::INFO_IDENTITY));
    }
    g->n_info += (none ? 0 : 1) - (g->has_info[e] ? 1 : 0);
    g->has_info[e] = none ? 0 : 1;
    memcpy(&g->info[(size_t)21 * e], none ? pg_g2o::INFO_IDENTITY : info21, sizeof(pg_g2o::INFO_IDENTITY));
    if (g->n_info == 0)
        pg_drop_info(g);  // all identity again: back to the identity kernel
    else if (e < g->dev_ninfo)
        g->dev_ninfo = 0;  // changed under an uploaded edge: the next solve uploads the buffer again
}

// a new edge was appended to efrom / eto / meas: the information vector, where one exists, follows
static void pg_append_info(svo_posegraph *g, const double *info21)
{
    if (!g->info.empty()) {
        g->has_info.push_back(0);
        g->info.insert(g->info.end(), pg_g2o::INFO_IDENTITY, pg_g2o::INFO_IDENTITY + 21);
    }
    pg_store_info(g, g->ne() - 1, info21);
}

static void pg_drop_robust(svo_posegraph *g)
{
    g->rkind.clear();
    g->rdelta.clear();
    g->n_robust = 0;
}

// Stores the (checked) kernel of edge e; NONE = none.  The edge must exist.
static void pg_store_robust(svo_posegraph *g, int e, int kind, double delta)
{
    const bool none = kind == SVO_PG_ROBUST_NONE;
    g->eo_w_ne = -1;
    if (g->rkind.empty()) {
        if (none)
            return;
        g->rkind.assign(g->ne(), SVO_PG_ROBUST_NONE);
        g->rdelta.assign(g->ne(), 0.);
    }
    g->n_robust += (none ? 0 : 1) - (g->rkind[e] != SVO_PG_ROBUST_NONE ? 1 : 0);
    g->rkind[e] = kind;
    g->rdelta[e] = none ? 0. : delta;
    if (g->n_robust == 0)
        pg_drop_robust(g);  // no kernel left: back to the non-robust linearisations
}

// a new edge was appended to efrom / eto / meas: the kernel vectors, where they exist, follow
static void pg_append_robust(svo_posegraph *g, int kind, double delta)
{
    if (!g->rkind.empty()) {
        g->rkind.push_back(SVO_PG_ROBUST_NONE);
        g->rdelta.push_back(0.);
    }
    pg_store_robust(g, g->ne() - 1, kind, delta);
}

// The graph itself on the device: grown buffers keep what the device already holds, only the tail is uploaded (poses, edges,
// measurements; with `weighted` the information; the robust kernels, where the graph stores any, whole: 12 bytes an edge).
// Queued on `st` from vectors that live in *g, so the copies need no sync.  The CALLER sets dev_nv / dev_ne / dev_ninfo to 0 until
// its work on the device has succeeded, and to nv / ne / (weighted ? ne : 0) then.
static int pg_upload_graph(svo_posegraph *g, const bool weighted, hipStream_t st)
{
    const int nv = g->nv(), ne = g->ne();
    int rc;
    if (g->dev_nv > nv || g->dev_ne > ne)
        g->dev_nv = g->dev_ne = 0;
    if ((rc = ensure_keep(g->d_pose, (size_t)nv * 56, (size_t)g->dev_nv * 56, st)) ||
        (rc = ensure_keep(g->d_from, (size_t)ne * 4, (size_t)g->dev_ne * 4, st)) ||
        (rc = ensure_keep(g->d_to, (size_t)ne * 4, (size_t)g->dev_ne * 4, st)) ||
        (rc = ensure_keep(g->d_meas, (size_t)ne * 56, (size_t)g->dev_ne * 56, st)))
        return rc;
    if (!weighted || g->dev_ninfo > ne || g->dev_ninfo > g->dev_ne)
        g->dev_ninfo = 0;
    if (weighted && (rc = ensure_keep(g->d_info, (size_t)ne * 168, (size_t)g->dev_ninfo * 168, st)))
        return rc;
    const bool robust = g->n_robust > 0;
    if (robust && ((rc = g->d_rkind.ensure((size_t)ne * 4)) || (rc = g->d_rdelta.ensure((size_t)ne * 8))))
        return rc;
    if (nv > g->dev_nv)
        SVO_HIP(hipMemcpyAsync(g->d_pose.as<double>() + 7 * (size_t)g->dev_nv, g->pose.data() + 7 * (size_t)g->dev_nv,
                               (size_t)(nv - g->dev_nv) * 56, hipMemcpyHostToDevice, st));
    if (ne > g->dev_ne) {
        const size_t e0 = (size_t)g->dev_ne, cnt = (size_t)(ne - g->dev_ne);
        SVO_HIP(hipMemcpyAsync(g->d_from.as<int>() + e0, g->efrom.data() + e0, cnt * 4, hipMemcpyHostToDevice, st));
        SVO_HIP(hipMemcpyAsync(g->d_to.as<int>() + e0, g->eto.data() + e0, cnt * 4, hipMemcpyHostToDevice, st));
        SVO_HIP(hipMemcpyAsync(g->d_meas.as<double>() + 7 * e0, g->meas.data() + 7 * e0, cnt * 56, hipMemcpyHostToDevice, st));
    }
    if (weighted && ne > g->dev_ninfo)
        SVO_HIP(hipMemcpyAsync(g->d_info.as<double>() + 21 * (size_t)g->dev_ninfo, g->info.data() + 21 * (size_t)g->dev_ninfo,
                               (size_t)(ne - g->dev_ninfo) * 168, hipMemcpyHostToDevice, st));
    if (robust) {
        SVO_HIP(hipMemcpyAsync(g->d_rkind.p, g->rkind.data(), (size_t)ne * 4, hipMemcpyHostToDevice, st));
        SVO_HIP(hipMemcpyAsync(g->d_rdelta.p, g->rdelta.data(), (size_t)ne * 8, hipMemcpyHostToDevice, st));
    }
    return SVO_OK;
}

// chi2 | w | rho of every edge at the current estimates -> res (3 ne doubles); one wait
static int pg_edge_eval(svo_posegraph *g, std::vector<double> &res)
{
    svo_ctx *ctx = g->ctx;
    SVO_HIP(hipSetDevice(ctx->device));
    const int nv = g->nv(), ne = g->ne();
    res.assign(3 * (size_t)ne, 0.);
    if (ne == 0)
        return SVO_OK;
    hipStream_t st = ctx->stream;
    const bool weighted = g->n_info > 0, robust = g->n_robust > 0;
    int rc;
    if ((rc = pg_upload_graph(g, weighted, st)) || (rc = g->d_eval.ensure(3 * (size_t)ne * 8)))
        return rc;
    g->dev_nv = g->dev_ne = g->dev_ninfo = 0;  // until the wait below has succeeded the device copy is not to be trusted
    const int *rk = robust ? g->d_rkind.as<int>() : nullptr;
    const double *rd = robust ? g->d_rdelta.as<double>() : nullptr;
    if (weighted)
        hipLaunchKernelGGL(pg_edge_eval_kernel<true>, dim3((ne + 127) / 128), dim3(128), 0, st, g->d_pose.as<double>(),
                           g->d_from.as<int>(), g->d_to.as<int>(), g->d_meas.as<double>(), ne, g->d_info.as<double>(), rk, rd,
                           g->d_eval.as<double>());
    else
        hipLaunchKernelGGL(pg_edge_eval_kernel<false>, dim3((ne + 127) / 128), dim3(128), 0, st, g->d_pose.as<double>(),
                           g->d_from.as<int>(), g->d_to.as<int>(), g->d_meas.as<double>(), ne, static_cast<const double *>(nullptr),
                           rk, rd, g->d_eval.as<double>());
    SVO_HIP(hipGetLastError());
    SVO_HIP(hipMemcpyAsync(res.data(), g->d_eval.p, 3 * (size_t)ne * 8, hipMemcpyDeviceToHost, st));
    SVO_HIP(hipStreamSynchronize(st));
    g->dev_nv = nv;
    g->dev_ne = ne;
    g->dev_ninfo = weighted ? ne : 0;
    return SVO_OK;
}

extern "C" {

int svo_pg_create(svo_ctx *ctx, svo_posegraph **out)
{
    SVO_CHECK_ARG(ctx && out);
    svo_posegraph *g = new svo_posegraph();
    g->ctx = ctx;
    if (const char *e = getenv("SVO_PG_REFINE"))
        g->refine = atoi(e) > 0 ? (atoi(e) > 4 ? 4 : atoi(e)) : 0;
    *out = g;
    return svo_pg_initialize(g);
}

int svo_pg_destroy(svo_posegraph *g)
{
    if (!g)
        return SVO_OK;
    (void)hipSetDevice(g->ctx->device);
    (void)hipStreamSynchronize(g->ctx->stream);
    DevBuf *bufs[] = {&g->d_rkind, &g->d_rdelta, &g->d_eval, &g->d_pose, &g->d_from, &g->d_to, &g->d_meas, &g->d_info, &g->d_eo,  &g->d_incptr, &g->d_inc, &g->d_struct,
                      &g->d_Dg,   &g->d_Cc,   &g->d_rneg, &g->d_Y,     &g->d_Wl,
                      &g->d_Wr,   &g->d_Wc,   &g->d_R,    &g->d_Lo, &g->d_Tinv, &g->d_rR,  &g->d_xR,  &g->d_misc, &g->d_dx, &g->d_res};
    for (DevBuf *b : bufs)
        b->release();
    delete g;
    return SVO_OK;
}

int svo_pg_initialize(svo_posegraph *g)
{
    SVO_CHECK_ARG(g);
    g->pose.assign({0, 0, 0, 0, 0, 0, 1});  // vertex 0: identity, fixed (poseGraph.h:69-84)
    g->efrom.clear();
    g->eto.clear();
    g->meas.clear();
    pg_drop_info(g);
    pg_drop_robust(g);
    g->lc_kind = SVO_PG_ROBUST_NONE;
    g->lc_delta = 0;
    g->eo_w_ne = -1;
    g->prev = 0;
    g->dev_nv = g->dev_ne = 0;
    g->built_nv = g->built_ne = -1;
    return SVO_OK;
}

int svo_pg_augment_node(svo_posegraph *g, const double *pose7)
{
    SVO_CHECK_ARG(g && pose7 && g->prev >= 0);
    double p[7];
    memcpy(p, pose7, sizeof(p));
    q_normalize(p + 3);
    g->pose.insert(g->pose.end(), p, p + 7);
    const int cur = g->nv() - 1;
    // measurement = prev^-1 * cur from the CURRENT estimates (poseGraph.h:97,102)
    double inv[7], z[7];
    se3_inv(&g->pose[7 * g->prev], inv);
    se3_mul(inv, &g->pose[7 * cur], z);
    q_normalize(z + 3);
    g->efrom.push_back(g->prev);
    g->eto.push_back(cur);
    g->meas.insert(g->meas.end(), z, z + 7);
    pg_append_info(g, nullptr);
    pg_append_robust(g, SVO_PG_ROBUST_NONE, 0.);  // an odometry edge never gets a kernel
    g->prev = cur;
    return SVO_OK;
}

int svo_pg_add_loop_closure(svo_posegraph *g, int from_id)
{
    SVO_CHECK_ARG(g && from_id >= 0 && from_id < g->nv() && g->prev >= 0);
    const double id[7] = {0, 0, 0, 0, 0, 0, 1};  // poseGraph.h:118-121: identity measurement
    g->efrom.push_back(g->prev);
    g->eto.push_back(from_id);
    g->meas.insert(g->meas.end(), id, id + 7);
    pg_append_info(g, nullptr);
    pg_append_robust(g, g->lc_kind, g->lc_delta);
    return SVO_OK;
}

int svo_pg_add_loop_closure_measured(svo_posegraph *g, int from_id, const double *meas7, const double *info21)
{
    SVO_CHECK_ARG(g && from_id >= 0 && from_id < g->nv() && g->prev >= 0);
    double z[7] = {0, 0, 0, 0, 0, 0, 1};
    if (meas7) {
        memcpy(z, meas7, sizeof(z));
        double nrm = 0;
        for (int k = 0; k < 7; k++) {
            if (!std::isfinite(z[k])) {
                svo_set_error("pose graph: closure %d -> %d: measurement entry %d is not finite", g->prev, from_id, k);
                return SVO_ERR_ARG;
            }
            nrm += k >= 3 ? z[k] * z[k] : 0.;
        }
        if (!(nrm > 0)) {
            svo_set_error("pose graph: closure %d -> %d: the measurement's quaternion is zero", g->prev, from_id);
            return SVO_ERR_ARG;
        }
        q_normalize(z + 3);
    }
    int rc;
    if (info21 && (rc = pg_check_info(info21, "new edge", g->ne())))
        return rc;
    g->efrom.push_back(g->prev);
    g->eto.push_back(from_id);
    g->meas.insert(g->meas.end(), z, z + 7);
    pg_append_info(g, info21);
    pg_append_robust(g, g->lc_kind, g->lc_delta);
    return SVO_OK;
}

int svo_pg_set_edge_information(svo_posegraph *g, int e, const double *info21)
{
    SVO_CHECK_ARG(g && e >= 0 && e < g->ne());
    int rc;
    if (info21 && (rc = pg_check_info(info21, "edge", e)))
        return rc;
    pg_store_info(g, e, info21);
    g->eo_w_ne = -1;
    return SVO_OK;
}

int svo_pg_get_edge_information(const svo_posegraph *g, int e, double *info21)
{
    SVO_CHECK_ARG(g && e >= 0 && e < g->ne() && info21);
    memcpy(info21, g->info.empty() ? pg_g2o::INFO_IDENTITY : &g->info[(size_t)21 * e], sizeof(pg_g2o::INFO_IDENTITY));
    return SVO_OK;
}

int svo_pg_augment_nodes(svo_posegraph *g, int n, const double *pose7, const int *closure_from)
{
    SVO_CHECK_ARG(g && n >= 0 && (n == 0 || pose7));
    for (int i = 0; i < n; i++) {
        int rc;
        if (closure_from && closure_from[i] >= 0 && (rc = svo_pg_add_loop_closure(g, closure_from[i])))
            return rc;
        if ((rc = svo_pg_augment_node(g, pose7 + 7 * (size_t)i)))
            return rc;
    }
    return SVO_OK;
}

int svo_pg_set_refinement(svo_posegraph *g, int passes)
{
    SVO_CHECK_ARG(g && passes >= 0 && passes <= 4);
    g->refine = passes;
    return SVO_OK;
}

int svo_pg_num_vertices(const svo_posegraph *g) { return g ? g->nv() : 0; }
int svo_pg_num_edges(const svo_posegraph *g) { return g ? g->ne() : 0; }

int svo_pg_get_estimates(const svo_posegraph *g, double *pose7_out)
{
    SVO_CHECK_ARG(g && pose7_out);
    memcpy(pose7_out, g->pose.data(), g->pose.size() * sizeof(double));
    return SVO_OK;
}

int svo_pg_get_edge(const svo_posegraph *g, int e, int *from, int *to, double *meas7)
{
    SVO_CHECK_ARG(g && e >= 0 && e < g->ne());
    if (from)
        *from = g->efrom[e];
    if (to)
        *to = g->eto[e];
    if (meas7)
        memcpy(meas7, &g->meas[7 * e], 7 * sizeof(double));
    return SVO_OK;
}

int svo_pg_optimize(svo_posegraph *g, int iters, double *chi2)
{
    SVO_CHECK_ARG(g && iters >= 0);
    svo_ctx *ctx = g->ctx;
    SVO_HIP(hipSetDevice(ctx->device));
    const int nv = g->nv(), ne = g->ne(), nb = nv - 1;
    if (nb <= 0 || ne == 0) {
        if (chi2)
            for (int i = 0; i <= iters; i++)
                chi2[i] = 0;
        return SVO_OK;
    }
    // ---- structure (host, pg_solve_plan.hip.h): incidence lists, separators, segments, gather lists; rebuilt only when the
    // graph grew since the last solve.  SVO_PG_COVER=1 / 0 forces the cover / both ends (the tests run both).
    const bool rebuild = g->built_nv != nv || g->built_ne != ne;
    if (rebuild) {
        const char *force = getenv("SVO_PG_COVER");
        pg_solve_plan::build(nv, ne, g->efrom.data(), g->eto.data(), !force ? -1 : force[0] == '0' ? 0 : 1, g->plan);
    }
    const pg_solve_plan::Plan &plan = g->plan;
    if (const int bound = pg_solve_plan::solve_lds_refusal(plan)) {
        svo_set_error("pose graph: %d separators -- the distinct loop-closure endpoints plus one regular separator per %d vertices "
                      "of a run without one -- are more than the separator solve holds in one workgroup's LDS (%d)", plan.m, SEG_L,
                      bound);
        return SVO_ERR_ARG;
    }
    hipStream_t st = ctx->stream;
    int rc;
    // the weighted linearisation runs only for a graph that stores at least one non-identity information matrix, the robust
    // ones only for a graph that stores at least one kernel
    const bool weighted = g->n_info > 0, robust = g->n_robust > 0;
    g->eo_w_ne = -1;
    if ((rc = g->d_eo.ensure((size_t)ne * EO_FIELDS * 8)) || (rc = g->d_incptr.ensure((size_t)(nv + 1) * 4)) ||
        (rc = g->d_inc.ensure((size_t)2 * ne * 4)) || (rc = g->d_struct.ensure(plan.buf.size() * 4 + 16)) ||
        (rc = g->d_Dg.ensure((size_t)nb * 288)) || (rc = g->d_Cc.ensure((size_t)nb * 288)) ||
        (rc = g->d_rneg.ensure((size_t)nb * 48)) || (rc = g->d_dx.ensure((size_t)nb * 48)) || (rc = g->d_res.ensure((size_t)nb * 48)) ||
        (rc = g->d_Y.ensure((size_t)nb * 48)) || (rc = g->d_Wl.ensure((size_t)nb * 288)) ||
        (rc = g->d_Wr.ensure((size_t)nb * 288)) || (rc = g->d_Wc.ensure(plan.wc_blocks * 288 + 64)) ||
        (rc = g->d_R.ensure((size_t)plan.ldr * plan.ldr * 8 + 64)) || (rc = g->d_Lo.ensure((size_t)plan.ldr * plan.ldr * 8 + 64)) ||
        (rc = g->d_Tinv.ensure((size_t)2 * (plan.T + 1) * TB * TB * 8 + 64)) ||
        (rc = g->d_rR.ensure((size_t)plan.ldr * 8 + 64)) || (rc = g->d_xR.ensure((size_t)plan.ldr * 8 + 64)) ||
        (rc = g->d_misc.ensure(((size_t)iters + 6 + (ne + 127) / 128) * 8 + 64)))
        return rc;
    // (g->pose / efrom / eto / meas and the plan's vectors live in *g: the copies need no sync)
    if ((rc = pg_upload_graph(g, weighted, st)))
        return rc;
    if (rebuild) {
        SVO_HIP(hipMemcpyAsync(g->d_incptr.p, plan.incptr.data(), (size_t)(nv + 1) * 4, hipMemcpyHostToDevice, st));
        SVO_HIP(hipMemcpyAsync(g->d_inc.p, plan.inc.data(), (size_t)2 * ne * 4, hipMemcpyHostToDevice, st));
        SVO_HIP(hipMemcpyAsync(g->d_struct.p, plan.buf.data(), plan.buf.size() * 4, hipMemcpyHostToDevice, st));
        g->built_nv = nv;
        g->built_ne = ne;
    }
    g->dev_nv = g->dev_ne = g->dev_ninfo = 0;  // until this solve has succeeded the device copy is not to be trusted
    const int *ds = g->d_struct.as<int>();
    double *d_chi = g->d_misc.as<double>();
    int *d_status = reinterpret_cast<int *>(d_chi + iters + 2);
    unsigned *d_ticket = reinterpret_cast<unsigned *>(d_chi + iters + 3);
    double *d_part = d_chi + iters + 4;  // chi2 per linearize workgroup
    SVO_HIP(hipMemsetAsync(d_status, 0, 16, st));  // status and ticket
    double *eo = g->d_eo.as<double>();
    double *Dg = g->d_Dg.as<double>(), *Cc = g->d_Cc.as<double>(), *rneg = g->d_rneg.as<double>();
    double *Y = g->d_Y.as<double>(), *Wl = g->d_Wl.as<double>(), *Wr = g->d_Wr.as<double>(), *Wc = g->d_Wc.as<double>();
    const PgSegChords seg_chords = {ds + plan.o_cptr, ds + plan.o_clrow, ds + plan.o_cedge, ds + plan.o_ctr, ds + plan.o_cwbase};
    double *R = g->d_R.as<double>(), *Lo = g->d_Lo.as<double>(), *Tinv = g->d_Tinv.as<double>();
    double *rR = g->d_rR.as<double>(), *xR = g->d_xR.as<double>();
    // the separator solve keeps its vector and its running sums in LDS (what does not fit was refused above)
    const size_t solve_lds = (size_t)(2 * plan.ldr + TB) * 8;
    if (solve_lds > 48 * 1024)
        SVO_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(pg_dense_solve_kernel),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)solve_lds));
    // a segment's rows live in LDS: SEG_L - 1 of them between two regular separators, SEG_L in a tail segment (the
    // regular-separator loop stops one row before the end) -- ADVICE r4: the bound to check is SEG_L itself
    static_assert(SEG_L <= BCR_MAX_ROWS, "a segment must fit the LDS of one workgroup");
    const size_t seg_lds = (size_t)plan.maxseg * BCR_ROW * 8;
    if (seg_lds > 48 * 1024)
        SVO_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(pg_segment_kernel),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)seg_lds));
    ScopedKernelTime tm(ctx, SVO_K_POSEGRAPH);
    for (int it = 0; it <= iters; it++) {
        auto linearize = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3((ne + 127) / 128), dim3(128), 0, st, g->d_pose.as<double>(), g->d_from.as<int>(),
                               g->d_to.as<int>(), g->d_meas.as<double>(), ne, eo, d_part, d_ticket, d_chi + it,
                               weighted ? g->d_info.as<double>() : static_cast<const double *>(nullptr),
                               robust ? g->d_rkind.as<int>() : static_cast<const int *>(nullptr),
                               robust ? g->d_rdelta.as<double>() : static_cast<const double *>(nullptr));
        };
        if (robust)
            weighted ? linearize(pg_linearize_kernel<true, true>) : linearize(pg_linearize_kernel<false, true>);
        else
            weighted ? linearize(pg_linearize_kernel<true, false>) : linearize(pg_linearize_kernel<false, false>);
        if (it == iters)
            break;
        hipLaunchKernelGGL(pg_assemble_kernel, dim3((nb + PG_ASM_ROWS - 1) / PG_ASM_ROWS), dim3(PG_ASM_ROWS * 78), 0, st, nb,
                           g->d_incptr.as<int>(), g->d_inc.as<int>(), g->d_from.as<int>(), g->d_to.as<int>(), eo, Dg, Cc,
                           rneg);
        // the linear solve H dx = rneg; with refinement (g->refine passes) again for the residual of what it returned
        const double *rhs = rneg;
        for (int pass = 0; pass <= g->refine; pass++) {
            const bool last = pass == g->refine;
            if (plan.nseg > 0 || plan.m > 0)
                hipLaunchKernelGGL(pg_segment_kernel, dim3(plan.nseg + (plan.m > 0 ? PG_CLEAR_WGS : 0)), dim3(BCR_WAVES * 64),
                                   seg_lds, st, nb, plan.nseg, ds + plan.o_seg_start, ds + plan.o_seg_len, Dg, Cc, rhs, Y, Wl, Wr,
                                   d_status, R, plan.ldr, 6 * plan.m, rR, seg_chords, eo, Wc);
            if (plan.m > 0) {
                static_assert(sizeof(psp::Src) == sizeof(int2) && offsetof(psp::Src, kind) == offsetof(int2, x) &&
                                  offsetof(psp::Src, idx) == offsetof(int2, y), "the kernel reads a source as an int2");
                hipLaunchKernelGGL(pg_reduce_kernel, dim3(plan.nrblocks + plan.m), dim3(64), 0, st, plan.nrblocks, plan.m,
                                   ds + plan.o_rb_row, ds + plan.o_rb_col, ds + plan.o_rptr,
                                   reinterpret_cast<const int2 *>(ds + plan.o_rsrc),
                                   reinterpret_cast<const PgTerm *>(ds + plan.o_terms), Dg, Cc, rhs, eo, Y, Wl, Wr, Wc, R, plan.ldr,
                                   rR);
                double *Tp = Tinv + (size_t)(plan.T + 1) * TB * TB;  // the inverses again, in the solve's layout
                hipLaunchKernelGGL(pg_dense_potf2_kernel, dim3(1), dim3(256), 0, st, R, Tinv, Tp, plan.ldr, 0, d_status, 1 << 20);
                for (int kb = 0; kb + 1 < plan.T; kb++) {
                    const int nt = plan.T - 1 - kb;
                    hipLaunchKernelGGL(pg_dense_step_kernel, dim3(nt * (nt + 1) / 2 + 1), dim3(256), 0, st, R, Lo, Tinv, Tp, plan.ldr,
                                       plan.T, kb, rR, xR, d_status, 1 << 20);
                }
                hipLaunchKernelGGL(pg_dense_solve_kernel, dim3(1), dim3(PG_SOLVE_THREADS), solve_lds, st, Lo, Tinv, Tp, plan.ldr,
                                   plan.T, rR, xR);
            }
            double *dxs = g->d_dx.as<double>();
            hipLaunchKernelGGL(pg_backsub_update_kernel, dim3((nb + PG_UPD_ROWS - 1) / PG_UPD_ROWS), dim3(PG_UPD_ROWS * 6), 0, st,
                               nb, ds + plan.o_sepidx, ds + plan.o_lsep, ds + plan.o_rsep, xR, Y, Wl, Wr, ds + plan.o_rowseg,
                               ds + plan.o_seg_start, ds + plan.o_cptr, ds + plan.o_csep, ds + plan.o_cwbase, Wc,
                               g->d_pose.as<double>(), pass > 0 ? dxs : nullptr, last ? nullptr : dxs);
            if (!last) {
                hipLaunchKernelGGL(pg_residual_kernel, dim3((nb + PG_UPD_ROWS - 1) / PG_UPD_ROWS), dim3(PG_UPD_ROWS * 6), 0, st, nb,
                                   g->d_incptr.as<int>(), g->d_inc.as<int>(), g->d_from.as<int>(), g->d_to.as<int>(), eo, rneg, dxs,
                                   g->d_res.as<double>());
                rhs = g->d_res.as<double>();
            }
        }
    }
    SVO_HIP(hipGetLastError());
    // the optimised poses go into a temporary: a failed solve must not destroy the caller's estimate
    std::vector<double> hpose((size_t)nv * 7);
    SVO_HIP(hipMemcpyAsync(hpose.data(), g->d_pose.p, (size_t)nv * 56, hipMemcpyDeviceToHost, st));
    std::vector<double> hchi(iters + 1);
    SVO_HIP(hipMemcpyAsync(hchi.data(), d_chi, (size_t)(iters + 1) * 8, hipMemcpyDeviceToHost, st));
    int hstatus = 0;
    SVO_HIP(hipMemcpyAsync(&hstatus, d_status, 4, hipMemcpyDeviceToHost, st));
    SVO_HIP(hipStreamSynchronize(st));
    if (chi2)
        memcpy(chi2, hchi.data(), (size_t)(iters + 1) * 8);
    if (iters > 0 && hstatus != 0) {
        if (hstatus >= (1 << 20))
            svo_set_error("pose graph: reduced (separator) system not positive definite at row %d",
                          hstatus - (1 << 20) - 1);
        else
            svo_set_error("pose graph: normal matrix not positive definite at block row %d", hstatus - 1);
        return SVO_ERR_STATE;
    }
#ifdef PG_STAMPS
    {
        long long h[128];
        (void)hipMemcpyFromSymbol(h, HIP_SYMBOL(pg_dbg), sizeof(h));
        fprintf(stderr, "first tile, us:");
        for (int k = 1; k <= 51; k++)
            if (h[k])
                fprintf(stderr, " [%d]%.2f", k, (h[k] - h[0]) * 0.01);
        fprintf(stderr, "\nfirst step, workgroup 0, us:");
        for (int k = 61; k <= 66; k++)
            fprintf(stderr, " [%d]%.2f", k, (h[k] - h[60]) * 0.01);
        fprintf(stderr, "\nseparator solve, us (start of step i, x_i known):");
        for (int k = 100; k <= 127; k++)
            if (h[k])
                fprintf(stderr, " [%d]%.2f", k, (h[k] - h[99]) * 0.01);
        fprintf(stderr, "\na long segment, us:");
        for (int k = 71; k <= 97; k++)
            if (h[k])
                fprintf(stderr, " [%d]%.2f", k, (h[k] - h[70]) * 0.01);
        fprintf(stderr, "\n");
    }
#endif
    g->pose.swap(hpose);
    g->dev_nv = nv;  // device poses == host poses, edges unchanged: the next solve uploads what is appended
    g->dev_ne = ne;
    g->dev_ninfo = weighted ? ne : 0;
    g->eo_w_ne = robust ? ne : -1;
    return SVO_OK;
}

int svo_pg_write_g2o(const svo_posegraph *g, const char *path)
{
    SVO_CHECK_ARG(g && path);
    FILE *f = fopen(path, "w");
    if (!f) {
        svo_set_error("cannot open %s", path);
        return SVO_ERR_ARG;
    }
    for (int v = 0; v < g->nv(); v++) {
        const double *p = &g->pose[7 * v];
        fprintf(f, "VERTEX_SE3:QUAT %d %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", v, p[0], p[1], p[2], p[3], p[4],
                p[5], p[6]);
    }
    for (int e = 0; e < g->ne(); e++) {
        const double *z = &g->meas[7 * e];
        fprintf(f, "EDGE_SE3:QUAT %d %d %.17g %.17g %.17g %.17g %.17g %.17g %.17g", g->efrom[e], g->eto[e], z[0], z[1],
                z[2], z[3], z[4], z[5], z[6]);
        if (!g->info.empty() && g->has_info[e])
            for (int k = 0; k < 21; k++)
                fprintf(f, " %.17g", g->info[(size_t)21 * e + k]);
        else  // no stored information: the integers of the identity, as the reference's files have them
            for (int i = 0; i < 6; i++)
                for (int j = i; j < 6; j++)
                    fprintf(f, " %d", i == j ? 1 : 0);
        fprintf(f, "\n");
    }
    fclose(f);
    return SVO_OK;
}

// The inverse of svo_pg_write_g2o / saveStructure: replaces the graph by the file's content (pg_g2o::read has the format and the
// refusals); keep_info: the edges' 21 information numbers are kept, else ignored as the reference leaves them at identity.
static int pg_read_g2o(svo_posegraph *g, const char *path, const bool keep_info)
{
    SVO_CHECK_ARG(g && path);
    pg_g2o::Graph in;
    const std::string why = pg_g2o::read(path, keep_info, in);
    if (!why.empty()) {
        svo_set_error("%s", why.c_str());
        return SVO_ERR_ARG;
    }
    g->pose.swap(in.pose);
    g->efrom.swap(in.efrom);
    g->eto.swap(in.eto);
    g->meas.swap(in.meas);
    pg_drop_info(g);
    pg_drop_robust(g);  // (the format has no field for kernels)
    g->lc_kind = SVO_PG_ROBUST_NONE;
    g->lc_delta = 0;
    g->eo_w_ne = -1;
    for (size_t e = 0; e < in.has_info.size(); e++)
        if (in.has_info[e])
            pg_store_info(g, (int)e, &in.info[21 * e]);
    g->prev = g->nv() - 1;
    g->dev_nv = g->dev_ne = 0;
    g->built_nv = g->built_ne = -1;
    return SVO_OK;
}

int svo_pg_read_g2o(svo_posegraph *g, const char *path) { return pg_read_g2o(g, path, false); }
int svo_pg_read_g2o_info(svo_posegraph *g, const char *path) { return pg_read_g2o(g, path, true); }

// ---- robust kernels and pruning ----------------------------------------------------------------
int svo_pg_set_robust_kernel(svo_posegraph *g, int e, int kind, double delta)
{
    SVO_CHECK_ARG(g && e >= 0 && e < g->ne());
    if (const char *why = pg_prune_plan::check_kernel(kind, delta)) {
        svo_set_error("svo_pg_set_robust_kernel: edge %d: %s (kind %d, parameter %g)", e, why, kind, delta);
        return SVO_ERR_ARG;
    }
    pg_store_robust(g, e, kind, delta);
    return SVO_OK;
}

int svo_pg_get_robust_kernel(const svo_posegraph *g, int e, int *kind, double *delta)
{
    SVO_CHECK_ARG(g && e >= 0 && e < g->ne());
    if (kind)
        *kind = g->rkind.empty() ? SVO_PG_ROBUST_NONE : g->rkind[e];
    if (delta)
        *delta = g->rdelta.empty() ? 0. : g->rdelta[e];
    return SVO_OK;
}

int svo_pg_set_loop_closure_kernel(svo_posegraph *g, int kind, double delta)
{
    SVO_CHECK_ARG(g);
    if (const char *why = pg_prune_plan::check_kernel(kind, delta)) {
        svo_set_error("svo_pg_set_loop_closure_kernel: %s (kind %d, parameter %g)", why, kind, delta);
        return SVO_ERR_ARG;
    }
    g->lc_kind = kind;
    g->lc_delta = kind == SVO_PG_ROBUST_NONE ? 0. : delta;
    return SVO_OK;
}

int svo_pg_edge_residuals(svo_posegraph *g, double *chi2, double *weight, double *rho)
{
    SVO_CHECK_ARG(g);
    std::vector<double> res;
    int rc;
    if ((rc = pg_edge_eval(g, res)))
        return rc;
    const size_t ne = (size_t)g->ne();
    double *outs[3] = {chi2, weight, rho};
    for (int k = 0; k < 3; k++)
        if (outs[k] && ne)
            memcpy(outs[k], res.data() + k * ne, ne * sizeof(double));
    return SVO_OK;
}

int svo_pg_linearization_weights(svo_posegraph *g, double *weight)
{
    SVO_CHECK_ARG(g && weight);
    const int ne = g->ne();
    if (g->eo_w_ne != ne || ne == 0 || g->dev_ne != ne || g->dev_nv != g->nv()) {
        svo_set_error("svo_pg_linearization_weights: the last svo_pg_optimize used no robust kernel, or the graph has changed since");
        return SVO_ERR_STATE;
    }
    SVO_HIP(hipSetDevice(g->ctx->device));
    SVO_HIP(hipMemcpy2DAsync(weight, sizeof(double), g->d_eo.as<double>() + EO_W, EO_FIELDS * sizeof(double), sizeof(double),
                             (size_t)ne, hipMemcpyDeviceToHost, g->ctx->stream));
    SVO_HIP(hipStreamSynchronize(g->ctx->stream));
    return SVO_OK;
}

int svo_pg_prune_edges(svo_posegraph *g, double threshold, int *removed, int cap, int *n_removed)
{
    SVO_CHECK_ARG(g && cap >= 0 && (removed || cap == 0));
    if (n_removed)
        *n_removed = 0;
    if (std::isnan(threshold)) {
        svo_set_error("svo_pg_prune_edges: the threshold is NaN");
        return SVO_ERR_ARG;
    }
    if (g->n_robust == 0)
        return SVO_OK;  // no edge carries a kernel: nothing can go, and nothing is evaluated
    std::vector<double> res;
    int rc;
    if ((rc = pg_edge_eval(g, res)))
        return rc;
    const int ne = g->ne();
    pg_prune_plan::Plan plan;
    const int verdict = pg_prune_plan::plan(g->nv(), ne, g->efrom.data(), g->eto.data(), g->rkind.data(), res.data() + ne, threshold,
                                            cap, plan);
    if (n_removed)
        *n_removed = (int)plan.removed.size();
    if (verdict == pg_prune_plan::PRUNE_CAPACITY) {
        svo_set_error("svo_pg_prune_edges: %zu edges are below the threshold, `removed` holds %d", plan.removed.size(), cap);
        return SVO_ERR_CAPACITY;
    }
    if (verdict == pg_prune_plan::PRUNE_DISCONNECTS) {
        svo_set_error("svo_pg_prune_edges: without the %zu edges below the threshold vertex %d cannot be reached from vertex 0",
                      plan.removed.size(), plan.orphan);
        return SVO_ERR_STATE;
    }
    if (plan.removed.empty())
        return SVO_OK;
    memcpy(removed, plan.removed.data(), plan.removed.size() * sizeof(int));
    pg_prune_plan::compact(g->efrom, 1, plan.remap);
    pg_prune_plan::compact(g->eto, 1, plan.remap);
    pg_prune_plan::compact(g->meas, 7, plan.remap);
    if (!g->info.empty()) {
        pg_prune_plan::compact(g->info, 21, plan.remap);
        pg_prune_plan::compact(g->has_info, 1, plan.remap);
        g->n_info = 0;
        for (char h : g->has_info)
            g->n_info += h ? 1 : 0;
        if (g->n_info == 0)
            pg_drop_info(g);
    }
    pg_prune_plan::compact(g->rkind, 1, plan.remap);
    pg_prune_plan::compact(g->rdelta, 1, plan.remap);
    g->n_robust -= (int)plan.removed.size();  // every removed edge carried a kernel
    if (g->n_robust == 0)
        pg_drop_robust(g);
    // the device copies of the edges and the elimination structure are those of the graph before: the next solve uploads and
    // rebuilds (the poses did not change, but dev_nv and dev_ne go together)
    g->dev_nv = g->dev_ne = g->dev_ninfo = 0;
    g->built_nv = g->built_ne = -1;
    g->eo_w_ne = -1;
    return SVO_OK;
}

}  // extern "C"
