// cloud.hip -- a resident, indexed target cloud (svo_cloud) and what the Python prototype's PoseGraphOptimize does with
// one (src/ROSslam.py:34-73): point-to-plane ICP (open3d registration_icp as recalled) and the information matrix of
// the edge (get_information_matrix_from_point_clouds).  tests/icp_numpy.py restates every operation below; the two
// agree bit for bit (DESIGN.md section 10i lists the recalled points and the deviations).
//
// The index is sor_grid.hip's (cloud_index.hip.h): Morton order and three levels of 64-way boxes, built once per
// cloud.  What is new is the search, which returns INDICES:
//   * one wave per query; the query in double; the squared distance to a target point t is (dx dx + dy dy) + dz dz with
//     dx = p - (double)t, in double; candidates are ordered by (d2, index in the cloud's ORIGINAL order);
//   * the hierarchy is walked best-first per level: of the children that cannot be excluded the one with the smallest
//     bound is entered first, so the threshold tightens early.  A box is excluded only when a lower bound of the double
//     squared distance of any point inside it (box_mind2_d, shrunk by 1e-6 relative and 1e-300 absolute -- the
//     expression's own rounding is below 1e-15 relative) is not below the current threshold; the bound is STRICTLY
//     below the distance of every point in the box, so a point that ties the threshold is never excluded and the
//     result equals brute force over the whole cloud, ties included.  Every loop retires one lane per turn: at most
//     16 x 64 x 64 leaf visits per query;
//   * 1-NN (icp_nn_kernel): threshold = the best d2 so far, max_dist^2 at the start; a candidate wins when d2 is smaller,
//     or equal with a lower index than a winner already found (so d2 == max_dist^2 never corresponds: strict <);
//   * kNN (cloud_knn_kernel): the k best so far live one per lane, sorted; a leaf's 64 candidates that beat the k-th are
//     merged through LDS by rank counting (keys are distinct, so ranks are a permutation).
//
// Sums over correspondences (icp_terms_kernel, icp_finish_kernel) are in double on one fixed tree, the same for every
// launch geometry: source point i is leaf i (zero without a correspondence); leaves 64 w .. 64 w + 63 are summed by the
// halving tree s[l] += s[l + off], off = 32, 16, .. 1; the results B_w, padded with zeros to a multiple of 64, are summed
// 64 at a time by the same halving tree, and those results C_g are added in order of g to an accumulator that starts
// at 0.  No floating-point atomics anywhere.
//
// The whole registration is queued at once: per iteration the search (which first moves the source by the pending
// update), the terms and ONE wave that finishes the sums, tests convergence, solves the 6 x 6 system (Cholesky in a
// fixed order), builds the update and composes T.  After the stop every later kernel leaves at its first
// instruction, and the host waits once.
#include "cloud_index.hip.h"
#include "ransac_common.hip.h"

#define SVO_CLOUD_MAX_N (1 << 22)

struct svo_cloud {
    svo_ctx *ctx = nullptr;
    int n = 0;
    char *block = nullptr;  // one allocation: everything below
    float *xyz = nullptr;   // n x 3, original order
    float *pts = nullptr;   // n x 3, Morton order
    int *idx = nullptr;     // sorted position -> original index
    float *b1 = nullptr, *b2 = nullptr, *b3 = nullptr;
    double *normals = nullptr;  // n x 3, original order
    int *knn = nullptr;         // n x 64 at most: the neighbour lists of the last normals / kNN call
    int *d_m = nullptr;         // the size, on the device (the index kernels read it there)
    bool has_normals = false;
};

namespace {

constexpr double INF_D = __builtin_inf();
constexpr int NN_WAVES = 4;
constexpr int PSTRIDE = 32;  // doubles per partial record
constexpr int NV_ICP = 29;   // 21 J^T J, 6 J^T r, sum d2, count
constexpr int NV_INFO = 10;  // t0 t1 t2, t0 t0, t1 t1, t2 t2, t0 t1, t0 t2, t1 t2, count
constexpr int NV_EVAL = 2;   // sum d2, count
enum { MODE_ICP = 0, MODE_INFO = 1, MODE_EVAL = 2 };

struct CloudDev {
    const float *xyz, *pts;
    const int *idx;
    const float *b1, *b2, *b3;
    const double *normals;
    int n;
};

struct IcpState {
    double T[16];
    double upd[12];  // the pending update, 3 x 4: applied to the moved source by the next search
    double fitness, rmse;
    double JtJ[21], Jtr[6];
    double info[36];
    int iterations, done, n_corr, first;
};

struct Mat16 {
    double v[16];
};

// ---- the bound ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ double box_mind2_d(const float *__restrict__ box, int b, double px, double py, double pz)
{
    const double p[3] = {px, py, pz};
    double s = 0;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const double lo = box[6 * b + a], hi = box[6 * b + 3 + a], v = p[a];
        const double g = lo > v ? lo - v : (v > hi ? v - hi : 0.0);
        s += g * g;
    }
    return s;
}

__device__ __forceinline__ bool box_excluded(double mind2, double thr)
{
    return mind2 * (1.0 - 1e-6) - 1e-300 >= thr;
}

// the live child with the smallest bound among those that cannot be excluded, or -1
__device__ __forceinline__ int pick_child(bool live, double md, double thr)
{
    const bool cand = live && !box_excluded(md, thr);
    if (__ballot(cand) == 0)
        return -1;
    const double m = svo::wave_min(cand ? md : INF_D);
    const unsigned long long at_min = __ballot(cand && md == m);
    return __builtin_ctzll(at_min ? at_min : __ballot(cand));  // (no lane at the minimum: bounds that do not compare)
}

__device__ __forceinline__ bool less_di(double a, int ai, double b, int bi)
{
    return a < b || (a == b && ai < bi);
}

template <class V>
__device__ __forceinline__ void walk_hierarchy(const CloudDev &c, double px, double py, double pz, int lane, V &v)
{
    const int n1 = (c.n + 63) >> 6, n2 = (n1 + 63) >> 6, n3 = (n2 + 63) >> 6;  // n3 <= 16
    bool live3 = lane < n3;
    const double md3 = live3 ? box_mind2_d(c.b3, lane, px, py, pz) : INF_D;
    for (int k3; (k3 = pick_child(live3, md3, v.thr())) >= 0;) {
        live3 = live3 && lane != k3;
        const int c2 = k3 * 64 + lane;
        bool live2 = c2 < n2;
        const double md2 = live2 ? box_mind2_d(c.b2, c2, px, py, pz) : INF_D;
        for (int k2; (k2 = pick_child(live2, md2, v.thr())) >= 0;) {
            live2 = live2 && lane != k2;
            const int c1 = (k3 * 64 + k2) * 64 + lane;
            bool live1 = c1 < n1;
            const double md1 = live1 ? box_mind2_d(c.b1, c1, px, py, pz) : INF_D;
            for (int k1; (k1 = pick_child(live1, md1, v.thr())) >= 0;) {
                live1 = live1 && lane != k1;
                v.leaf(((k3 * 64 + k2) * 64 + k1) * 64);
            }
        }
    }
}

__device__ __forceinline__ double dist2_d(const float *__restrict__ pts, int j, double px, double py, double pz)
{
    const double dx = px - (double)pts[3 * j], dy = py - (double)pts[3 * j + 1], dz = pz - (double)pts[3 * j + 2];
    return (dx * dx + dy * dy) + dz * dz;
}

// ---- 1-NN within a radius -----------------------------------------------------------------------------------------
struct NearestVisitor {
    const CloudDev &c;
    double px, py, pz;
    int lane;
    double best_d;
    int best_i;
    __device__ __forceinline__ double thr() const { return best_d; }
    __device__ __forceinline__ void leaf(int base)
    {
        const int j = base + lane;
        double d = INF_D;
        int oi = 0x7fffffff;
        if (j < c.n) {
            d = dist2_d(c.pts, j, px, py, pz);
            oi = c.idx[j];
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const double od = __shfl_xor(d, off, 64);
            const int oo = __shfl_xor(oi, off, 64);
            if (less_di(od, oo, d, oi)) {
                d = od;
                oi = oo;
            }
        }
        if (d < best_d || (d == best_d && best_i >= 0 && oi < best_i)) {
            best_d = d;
            best_i = oi;
        }
    }
};

__device__ __forceinline__ void apply_rt(const double *__restrict__ m, int stride, double x, double y, double z,
                                         double &ox, double &oy, double &oz)
{
    ox = ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
    oy = ((m[stride] * x + m[stride + 1] * y) + m[stride + 2] * z) + m[stride + 3];
    oz = ((m[2 * stride] * x + m[2 * stride + 1] * y) + m[2 * stride + 2] * z) + m[2 * stride + 3];
}

// one wave per source point: move it (T src the first time, update pcd afterwards), then its correspondence
__global__ __launch_bounds__(64 * NN_WAVES) void icp_nn_kernel(const IcpState *__restrict__ st, const float *__restrict__ src,
                                                               double *__restrict__ pcd, int n_src, CloudDev c,
                                                               double max_d2, int *__restrict__ corr,
                                                               double *__restrict__ d2)
{
    if (st->done)
        return;
    const int lane = threadIdx.x & 63;
    const int i = __builtin_amdgcn_readfirstlane(blockIdx.x * NN_WAVES + (threadIdx.x >> 6));
    if (i >= n_src)
        return;
    double px, py, pz;
    if (st->first)
        apply_rt(st->T, 4, (double)src[3 * i], (double)src[3 * i + 1], (double)src[3 * i + 2], px, py, pz);
    else
        apply_rt(st->upd, 4, pcd[3 * i], pcd[3 * i + 1], pcd[3 * i + 2], px, py, pz);
    NearestVisitor v{c, px, py, pz, lane, max_d2, -1};
    if (fabs(px) < INF_D && fabs(py) < INF_D && fabs(pz) < INF_D)  // a non-finite moved point has no correspondence
        walk_hierarchy(c, px, py, pz, lane, v);
    if (lane == 0) {
        pcd[3 * i] = px;
        pcd[3 * i + 1] = py;
        pcd[3 * i + 2] = pz;
        corr[i] = v.best_i;
        d2[i] = v.best_i >= 0 ? v.best_d : 0.0;
    }
}

// ---- kNN with indices ---------------------------------------------------------------------------------------------
struct KnnLds {
    double md[128];
    double od[64];
    int mi[128];
    int oi[64];
};

struct KnnVisitor {
    const CloudDev &c;
    KnnLds &s;
    double px, py, pz;
    int lane, k;
    double cd;  // lane l: the l-th best so far (l < cnt)
    int ci;
    int cnt;
    double worst_d;
    int worst_i;
    __device__ __forceinline__ double thr() const { return worst_d; }
    __device__ __forceinline__ void leaf(int base)
    {
        const int j = base + lane;
        double d = INF_D;
        int oi = 0x7fffffff;
        bool acc = false;
        if (j < c.n) {
            d = dist2_d(c.pts, j, px, py, pz);
            oi = c.idx[j];
            acc = cnt < k || less_di(d, oi, worst_d, worst_i);
        }
        const unsigned long long bal = __ballot(acc);
        if (bal == 0)
            return;
        const bool mine = lane < cnt;
        const double d0 = mine ? cd : INF_D, d1 = acc ? d : INF_D;
        const int i0 = mine ? ci : 0x7fffffff, i1 = acc ? oi : 0x7fffffff;
        s.md[lane] = d0;
        s.mi[lane] = i0;
        s.md[64 + lane] = d1;
        s.mi[64 + lane] = i1;
        svo::wave_lds_fence();
        int r0 = 0, r1 = 0;
        for (int t = 0; t < 128; t++) {
            const double ed = s.md[t];
            const int ei = s.mi[t];
            r0 += less_di(ed, ei, d0, i0) ? 1 : 0;
            r1 += less_di(ed, ei, d1, i1) ? 1 : 0;
        }
        if (mine && r0 < k) {
            s.od[r0] = d0;
            s.oi[r0] = i0;
        }
        if (acc && r1 < k) {
            s.od[r1] = d1;
            s.oi[r1] = i1;
        }
        svo::wave_lds_fence();
        const int total = cnt + __popcll(bal);
        cnt = total < k ? total : k;
        if (lane < cnt) {
            cd = s.od[lane];
            ci = s.oi[lane];
        }
        if (cnt == k) {
            worst_d = __shfl(cd, k - 1, 64);
            worst_i = __shfl(ci, k - 1, 64);
        }
        svo::wave_lds_fence();
    }
};

// one wave per point, in Morton order; out[idx[i] * k + l] = its l-th neighbour, -1 past the end of a short list
__global__ __launch_bounds__(64 * NN_WAVES) void cloud_knn_kernel(CloudDev c, int k, int *__restrict__ out)
{
    __shared__ KnnLds s_lds[NN_WAVES];
    const int lane = threadIdx.x & 63;
    const int i = __builtin_amdgcn_readfirstlane(blockIdx.x * NN_WAVES + (threadIdx.x >> 6));
    if (i >= c.n)
        return;
    const double px = c.pts[3 * i], py = c.pts[3 * i + 1], pz = c.pts[3 * i + 2];
    KnnVisitor v{c, s_lds[threadIdx.x >> 6], px, py, pz, lane, k, INF_D, 0x7fffffff, 0, INF_D, 0x7fffffff};
    walk_hierarchy(c, px, py, pz, lane, v);
    if (lane < k)
        out[(size_t)c.idx[i] * k + lane] = lane < v.cnt ? v.ci : -1;
}

// ---- normals --------------------------------------------------------------------------------------------------------
// one rotation of the cyclic Jacobi method on the symmetric 3 x 3 matrix A (P < Q, R the third index), V <- V J
template <int P, int Q, int R>
__device__ __forceinline__ void jacobi_rot(double (&A)[3][3], double (&V)[3][3])
{
    const double apq = A[P][Q];
    if (apq == 0.0)
        return;
    const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (__builtin_fabs(theta) + __builtin_sqrt(theta * theta + 1.0));
    const double cs = 1.0 / __builtin_sqrt(t * t + 1.0), sn = t * cs;
    A[P][P] = A[P][P] - t * apq;
    A[Q][Q] = A[Q][Q] + t * apq;
    A[P][Q] = A[Q][P] = 0.0;
    const double arp = A[R][P], arq = A[R][Q];
    A[R][P] = A[P][R] = cs * arp - sn * arq;
    A[R][Q] = A[Q][R] = sn * arp + cs * arq;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const double vp = V[i][P], vq = V[i][Q];
        V[i][P] = cs * vp - sn * vq;
        V[i][Q] = sn * vp + cs * vq;
    }
}

constexpr int JACOBI_SWEEPS = 8;

__global__ __launch_bounds__(256) void cloud_normals_kernel(CloudDev c, int k, const int *__restrict__ knn,
                                                            double *__restrict__ normals)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= c.n)
        return;
    const int *nb = knn + (size_t)q * k;
    int cnt = 0;
    double mx = 0, my = 0, mz = 0;
    for (int l = 0; l < k; l++) {
        const int j = nb[l];
        if (j < 0)
            break;
        mx = mx + (double)c.xyz[3 * j];
        my = my + (double)c.xyz[3 * j + 1];
        mz = mz + (double)c.xyz[3 * j + 2];
        cnt++;
    }
    double nx = 0, ny = 0, nz = 1;
    if (cnt >= 3) {
        mx = mx / cnt;
        my = my / cnt;
        mz = mz / cnt;
        double A[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
        for (int l = 0; l < cnt; l++) {
            const int j = nb[l];
            const double dx = (double)c.xyz[3 * j] - mx, dy = (double)c.xyz[3 * j + 1] - my,
                         dz = (double)c.xyz[3 * j + 2] - mz;
            A[0][0] = A[0][0] + dx * dx;
            A[0][1] = A[0][1] + dx * dy;
            A[0][2] = A[0][2] + dx * dz;
            A[1][1] = A[1][1] + dy * dy;
            A[1][2] = A[1][2] + dy * dz;
            A[2][2] = A[2][2] + dz * dz;
        }
        A[1][0] = A[0][1];
        A[2][0] = A[0][2];
        A[2][1] = A[1][2];
        double V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
        for (int sweep = 0; sweep < JACOBI_SWEEPS; sweep++) {
            jacobi_rot<0, 1, 2>(A, V);
            jacobi_rot<0, 2, 1>(A, V);
            jacobi_rot<1, 2, 0>(A, V);
        }
        // the smallest eigenvalue, the lowest index on a tie
        double vx = V[0][0], vy = V[1][0], vz = V[2][0], ev = A[0][0];
        if (A[1][1] < ev) {
            ev = A[1][1];
            vx = V[0][1], vy = V[1][1], vz = V[2][1];
        }
        if (A[2][2] < ev) {
            ev = A[2][2];
            vx = V[0][2], vy = V[1][2], vz = V[2][2];
        }
        const double nrm = __builtin_sqrt((vx * vx + vy * vy) + vz * vz);
        if (nrm > 0.0 && nrm < INF_D) {
            nx = vx / nrm;
            ny = vy / nrm;
            nz = vz / nrm;
        }
    }
    normals[3 * q] = nx;
    normals[3 * q + 1] = ny;
    normals[3 * q + 2] = nz;
}

// ---- sums over correspondences ------------------------------------------------------------------------------------
template <int MODE> struct ModeNv {
    static constexpr int value = MODE == MODE_ICP ? NV_ICP : (MODE == MODE_INFO ? NV_INFO : NV_EVAL);
};

// leaf i of the tree = source point i; wave w sums leaves 64 w .. 64 w + 63 into partial[w]
template <int MODE>
__global__ __launch_bounds__(256) void icp_terms_kernel(const IcpState *__restrict__ st, const double *__restrict__ pcd,
                                                        const int *__restrict__ corr, const double *__restrict__ d2,
                                                        CloudDev c, int n_src, double *__restrict__ partial)
{
    constexpr int NV = ModeNv<MODE>::value;
    if (st->done)
        return;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    double v[NV];
#pragma unroll
    for (int k = 0; k < NV; k++)
        v[k] = 0.0;
    const int j = i < n_src ? corr[i] : -1;
    if (j >= 0) {
        const double t0 = c.xyz[3 * j], t1 = c.xyz[3 * j + 1], t2 = c.xyz[3 * j + 2];
        if constexpr (MODE == MODE_ICP) {
            const double s0 = pcd[3 * i], s1 = pcd[3 * i + 1], s2 = pcd[3 * i + 2];
            const double n0 = c.normals[3 * j], n1 = c.normals[3 * j + 1], n2 = c.normals[3 * j + 2];
            const double r = ((s0 - t0) * n0 + (s1 - t1) * n1) + (s2 - t2) * n2;
            const double J[6] = {s1 * n2 - s2 * n1, s2 * n0 - s0 * n2, s0 * n1 - s1 * n0, n0, n1, n2};
            int o = 0;
#pragma unroll
            for (int a = 0; a < 6; a++)
#pragma unroll
                for (int b = a; b < 6; b++)
                    v[o++] = J[a] * J[b];
#pragma unroll
            for (int a = 0; a < 6; a++)
                v[21 + a] = J[a] * r;
            v[27] = d2[i];
            v[28] = 1.0;
        } else if constexpr (MODE == MODE_INFO) {
            v[0] = t0;
            v[1] = t1;
            v[2] = t2;
            v[3] = t0 * t0;
            v[4] = t1 * t1;
            v[5] = t2 * t2;
            v[6] = t0 * t1;
            v[7] = t0 * t2;
            v[8] = t1 * t2;
            v[9] = 1.0;
        } else {
            v[0] = d2[i];
            v[1] = 1.0;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
        for (int k = 0; k < NV; k++)
            v[k] = v[k] + __shfl_down(v[k], off, 64);
    if (lane == 0 && i < n_src) {  // waves wholly past the end own no record
        double *p = partial + (size_t)(i >> 6) * PSTRIDE;
#pragma unroll
        for (int k = 0; k < NV; k++)
            p[k] = v[k];
    }
}

// Cholesky solve of the symmetric 6 x 6 system A x = b in a fixed order; false on a pivot <= 0 or a non-finite value
__device__ bool solve6(const double (&A)[6][6], const double (&b)[6], double (&x)[6])
{
    double L[6][6];
    for (int j = 0; j < 6; j++) {
        double s = A[j][j];
        for (int k = 0; k < j; k++)
            s = s - L[j][k] * L[j][k];
        if (!(s > 0.0) || !(s < INF_D))
            return false;
        L[j][j] = __builtin_sqrt(s);
        for (int i = j + 1; i < 6; i++) {
            double u = A[i][j];
            for (int k = 0; k < j; k++)
                u = u - L[i][k] * L[j][k];
            L[i][j] = u / L[j][j];
        }
    }
    double y[6];
    for (int i = 0; i < 6; i++) {
        double u = b[i];
        for (int k = 0; k < i; k++)
            u = u - L[i][k] * y[k];
        y[i] = u / L[i][i];
    }
    for (int i = 5; i >= 0; i--) {
        double u = y[i];
        for (int k = i + 1; k < 6; k++)
            u = u - L[k][i] * x[k];
        x[i] = u / L[i][i];
    }
    for (int i = 0; i < 6; i++)
        if (!(__builtin_fabs(x[i]) < INF_D))
            return false;
    return true;
}

// ONE wave: the upper levels of the tree, then (lane 0) what the mode asks for.  MODE_ICP: fitness and rmse of the
// correspondences just found; the convergence test against the previous ones (none the first time); unless stopped or
// `last`, the solve, the update and T <- update T.  MODE_INFO: Lambda.  MODE_EVAL: fitness and rmse.
template <int MODE>
__global__ __launch_bounds__(64) void icp_finish_kernel(IcpState *__restrict__ st, const double *__restrict__ partial,
                                                        int nw, int n_src, double rel_fitness, double rel_rmse, int last)
{
    constexpr int NV = ModeNv<MODE>::value;
    if (st->done)
        return;
    const int lane = threadIdx.x;
    double acc[NV];
#pragma unroll
    for (int k = 0; k < NV; k++)
        acc[k] = 0.0;
    for (int g = 0; g * 64 < nw; g++) {
        const int w = g * 64 + lane;
        double v[NV];
#pragma unroll
        for (int k = 0; k < NV; k++)
            v[k] = w < nw ? partial[(size_t)w * PSTRIDE + k] : 0.0;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
            for (int k = 0; k < NV; k++)
                v[k] = v[k] + __shfl_down(v[k], off, 64);
#pragma unroll
        for (int k = 0; k < NV; k++)
            acc[k] = acc[k] + v[k];
    }
    if (lane != 0)
        return;
    if constexpr (MODE == MODE_INFO) {
        const double t0 = acc[0], t1 = acc[1], t2 = acc[2], cnt = acc[9];
        double *M = st->info;
        for (int k = 0; k < 36; k++)
            M[k] = 0.0;
        M[0] = acc[4] + acc[5];
        M[7] = acc[3] + acc[5];
        M[14] = acc[3] + acc[4];
        M[1] = M[6] = -acc[6];
        M[2] = M[12] = -acc[7];
        M[8] = M[13] = -acc[8];
        M[4] = M[24] = -t2;
        M[5] = M[30] = t1;
        M[9] = M[19] = t2;
        M[11] = M[31] = -t0;
        M[15] = M[20] = -t1;
        M[16] = M[26] = t0;
        M[21] = M[28] = M[35] = cnt;
        st->n_corr = (int)cnt;
        st->done = 1;
        return;
    }
    const double cnt = acc[NV - 1], sum_d2 = acc[NV - 2];
    const double fitness = cnt / (double)n_src;
    const double rmse = cnt > 0.0 ? __builtin_sqrt(sum_d2 / cnt) : 0.0;
    bool stop = last != 0;
    if (!st->first && __builtin_fabs(fitness - st->fitness) < rel_fitness && __builtin_fabs(rmse - st->rmse) < rel_rmse)
        stop = true;
    st->fitness = fitness;
    st->rmse = rmse;
    st->n_corr = (int)cnt;
    st->first = 0;
    if (MODE == MODE_ICP) {
        for (int k = 0; k < 21; k++)
            st->JtJ[k] = acc[k];
        for (int k = 0; k < 6; k++)
            st->Jtr[k] = acc[21 + k];
    }
    if (MODE != MODE_ICP || stop) {
        st->done = 1;
        return;
    }
    double A[6][6], b[6], x[6];
    {
        int o = 0;
        for (int a = 0; a < 6; a++)
            for (int bb = a; bb < 6; bb++) {
                A[a][bb] = acc[o];
                A[bb][a] = acc[o];
                o++;
            }
    }
    for (int a = 0; a < 6; a++)
        b[a] = -acc[21 + a];
    double U[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    if (cnt > 0.0 && solve6(A, b, x)) {
        const double sx = svo_sin(x[0]), cx = svo_cos(x[0]), sy = svo_sin(x[1]), cy = svo_cos(x[1]), sz = svo_sin(x[2]),
                     cz = svo_cos(x[2]);
        U[0] = cz * cy;
        U[1] = (cz * sy) * sx - sz * cx;
        U[2] = (cz * sy) * cx + sz * sx;
        U[3] = x[3];
        U[4] = sz * cy;
        U[5] = (sz * sy) * sx + cz * cx;
        U[6] = (sz * sy) * cx - cz * sx;
        U[7] = x[4];
        U[8] = -sy;
        U[9] = cy * sx;
        U[10] = cy * cx;
        U[11] = x[5];
    }
    double Tn[12];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 4; j++) {
            double s = (U[4 * i] * st->T[j] + U[4 * i + 1] * st->T[4 + j]) + U[4 * i + 2] * st->T[8 + j];
            if (j == 3)
                s = s + U[4 * i + 3];
            Tn[4 * i + j] = s;
        }
    for (int k = 0; k < 12; k++) {
        st->T[k] = Tn[k];
        st->upd[k] = U[k];
    }
    st->iterations = st->iterations + 1;
}

__global__ void icp_init_kernel(IcpState *st, Mat16 T, const IcpState *from)
{
    if (blockIdx.x != 0 || threadIdx.x != 0)
        return;
    for (int k = 0; k < 16; k++)
        st->T[k] = from ? from->T[k] : T.v[k];
    st->T[12] = st->T[13] = st->T[14] = 0.0;
    st->T[15] = 1.0;
    for (int k = 0; k < 12; k++)
        st->upd[k] = (k % 5 == 0) ? 1.0 : 0.0;
    st->fitness = st->rmse = 0.0;
    for (int k = 0; k < 21; k++)
        st->JtJ[k] = 0.0;
    for (int k = 0; k < 6; k++)
        st->Jtr[k] = 0.0;
    for (int k = 0; k < 36; k++)
        st->info[k] = 0.0;
    st->iterations = 0;
    st->done = 0;
    st->n_corr = 0;
    st->first = 1;
}

// the first index with a non-finite coordinate (INT_MAX: none); an INTEGER atomic, order-free
__global__ __launch_bounds__(256) void cloud_check_kernel(const float *__restrict__ xyz, int n, int *__restrict__ bad)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    if (!(isfinite(xyz[3 * i]) && isfinite(xyz[3 * i + 1]) && isfinite(xyz[3 * i + 2])))
        atomicMin(bad, i);
}

CloudDev cloud_dev(const svo_cloud *c)
{
    return CloudDev{c->xyz, c->pts, c->idx, c->b1, c->b2, c->b3, c->normals, c->n};
}

// the work area of one registration call, carved from ctx->icp_work
struct IcpWork {
    float *src;
    double *pcd, *d2, *partial;
    int *corr;
    IcpState *st;  // [3]
    int nw;
};

int icp_work(svo_ctx *ctx, int n_src, IcpWork &w)
{
    const size_t n = (size_t)n_src;
    w.nw = (n_src + 63) / 64;
    size_t off = 0;
    const size_t o_src = off; off = align256(off + n * 12);
    const size_t o_pcd = off; off = align256(off + n * 24);
    const size_t o_d2 = off; off = align256(off + n * 8);
    const size_t o_corr = off; off = align256(off + n * 4);
    const size_t o_part = off; off = align256(off + (size_t)w.nw * PSTRIDE * 8);
    const size_t o_st = off; off = align256(off + 3 * sizeof(IcpState));
    int rc;
    if ((rc = ctx->icp_work.ensure(off)))
        return rc;
    char *g = ctx->icp_work.as<char>();
    w.src = reinterpret_cast<float *>(g + o_src);
    w.pcd = reinterpret_cast<double *>(g + o_pcd);
    w.d2 = reinterpret_cast<double *>(g + o_d2);
    w.corr = reinterpret_cast<int *>(g + o_corr);
    w.partial = reinterpret_cast<double *>(g + o_part);
    w.st = reinterpret_cast<IcpState *>(g + o_st);
    return SVO_OK;
}

void queue_search(svo_ctx *ctx, const IcpWork &w, const float *src, int n_src, const svo_cloud *t, double max_dist,
                  IcpState *st)
{
    hipLaunchKernelGGL(icp_nn_kernel, dim3((n_src + NN_WAVES - 1) / NN_WAVES), dim3(64 * NN_WAVES), 0, ctx->stream, st, src,
                       w.pcd, n_src, cloud_dev(t), max_dist * max_dist, w.corr, w.d2);
}

template <int MODE>
void queue_round(svo_ctx *ctx, const IcpWork &w, const float *src, int n_src, const svo_cloud *t, double max_dist,
                 const svo_icp_params &p, IcpState *st, int last)
{
    queue_search(ctx, w, src, n_src, t, max_dist, st);
    hipLaunchKernelGGL(icp_terms_kernel<MODE>, dim3((n_src + 255) / 256), dim3(256), 0, ctx->stream, st, w.pcd, w.corr,
                       w.d2, cloud_dev(t), n_src, w.partial);
    hipLaunchKernelGGL(icp_finish_kernel<MODE>, dim3(1), dim3(64), 0, ctx->stream, st, w.partial, w.nw, n_src,
                       p.relative_fitness, p.relative_rmse, last);
}

// every iteration of one registration: max_iteration rounds that may update, one that only evaluates
void queue_icp(svo_ctx *ctx, const IcpWork &w, const float *src, int n_src, const svo_cloud *t, double max_dist,
               const svo_icp_params &p, IcpState *st)
{
    for (int it = 0; it <= p.max_iteration; it++)
        queue_round<MODE_ICP>(ctx, w, src, n_src, t, max_dist, p, st, it == p.max_iteration);
}

int stage_source(svo_ctx *ctx, const IcpWork &w, const float *src_xyz, int n_src, int mem, const float **dev)
{
    if (mem == SVO_MEM_HOST) {
        SVO_HIP(hipMemcpyAsync(w.src, src_xyz, (size_t)n_src * 12, hipMemcpyHostToDevice, ctx->stream));
        *dev = w.src;
    } else {
        *dev = src_xyz;
    }
    return SVO_OK;
}

int check_call(svo_ctx *ctx, const float *src_xyz, int n_src, const svo_cloud *t, double max_dist, const double *T16,
               int mem, const char *who)
{
    SVO_CHECK_ARG(ctx && src_xyz && t && T16);
    SVO_CHECK_ARG(mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE);
    if (t->ctx != ctx) {
        svo_set_error("%s: the target cloud belongs to another context", who);
        return SVO_ERR_ARG;
    }
    if (n_src < 1 || n_src > SVO_CLOUD_MAX_N) {
        svo_set_error("%s: %d source points, 1 .. %d allowed", who, n_src, SVO_CLOUD_MAX_N);
        return SVO_ERR_ARG;
    }
    if (!(max_dist > 0.0) || !(max_dist < INF_D)) {
        svo_set_error("%s: max_dist %g must be positive and finite", who, max_dist);
        return SVO_ERR_ARG;
    }
    for (int k = 0; k < 12; k++)
        if (!(fabs(T16[k]) < INF_D)) {
            svo_set_error("%s: entry %d of the transform is not finite", who, k);
            return SVO_ERR_ARG;
        }
    return SVO_OK;
}

int check_params(const svo_icp_params *p, svo_icp_params &out, const char *who)
{
    svo_icp_default_params(&out);
    if (p)
        out = *p;
    if (out.max_iteration < 1 || out.max_iteration > 1000) {
        svo_set_error("%s: max_iteration %d outside 1 .. 1000", who, out.max_iteration);
        return SVO_ERR_ARG;
    }
    return SVO_OK;
}

int need_normals(const svo_cloud *t, const char *who)
{
    if (!t->has_normals) {
        svo_set_error("%s: the target cloud has no normals (svo_cloud_estimate_normals / svo_cloud_set_normals)", who);
        return SVO_ERR_STATE;
    }
    return SVO_OK;
}

Mat16 mat16(const double *T16)
{
    Mat16 m;
    for (int k = 0; k < 16; k++)
        m.v[k] = T16[k];
    return m;
}

// the states of a call -> pinned host memory, the one wait, the optional correspondences
int finish_call(svo_ctx *ctx, const IcpWork &w, int n_states, int n_src, int *corr_out, int mem, const IcpState **host)
{
    SVO_HIP(hipMemcpyAsync(ctx->pinned, w.st, n_states * sizeof(IcpState), hipMemcpyDeviceToHost, ctx->stream));
    if (corr_out)
        SVO_HIP(hipMemcpyAsync(corr_out, w.corr, (size_t)n_src * 4,
                               mem == SVO_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, ctx->stream));
    SVO_HIP(hipGetLastError());
    SVO_HIP(hipStreamSynchronize(ctx->stream));
    *host = reinterpret_cast<const IcpState *>(ctx->pinned);
    return SVO_OK;
}

}  // namespace

// ---- the cloud ------------------------------------------------------------------------------------------------------
extern "C" int svo_cloud_create(svo_ctx *ctx, const float *xyz, int n, int mem, svo_cloud **out)
{
    SVO_CHECK_ARG(ctx && out);
    *out = nullptr;
    SVO_CHECK_ARG(mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE);
    if (n < 1 || n > SVO_CLOUD_MAX_N) {
        svo_set_error("svo_cloud_create: %d points, 1 .. %d allowed", n, SVO_CLOUD_MAX_N);
        return SVO_ERR_ARG;
    }
    SVO_CHECK_ARG(xyz);
    const size_t N = (size_t)n;
    const int nb1 = (n + 63) / 64, nb2 = (nb1 + 63) / 64, nb3 = (nb2 + 63) / 64;
    const int nblk = (n + RS_TILE - 1) / RS_TILE;
    size_t off = 0;
    const size_t o_xyz = off; off = align256(off + N * 12);
    const size_t o_pts = off; off = align256(off + N * 12);
    const size_t o_idx = off; off = align256(off + N * 4);
    const size_t o_b1 = off; off = align256(off + (size_t)nb1 * 24);
    const size_t o_b2 = off; off = align256(off + (size_t)nb2 * 24);
    const size_t o_b3 = off; off = align256(off + (size_t)nb3 * 24);
    const size_t o_nrm = off; off = align256(off + N * 24);
    const size_t o_knn = off; off = align256(off + N * 64 * 4);
    const size_t o_m = off; off = align256(off + 64);
    const size_t keep = off;
    // the sort's buffers, freed before the call returns
    size_t toff = 0;
    const size_t o_k0 = toff; toff = align256(toff + N * 8);
    const size_t o_k1 = toff; toff = align256(toff + N * 8);
    const size_t o_v1 = toff; toff = align256(toff + N * 4);
    const size_t o_hist = toff; toff = align256(toff + (size_t)256 * nblk * 4);
    const size_t o_bnd = toff; toff = align256(toff + 64);
    char *g = nullptr, *tmp = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&g), keep);
    if (e == hipSuccess)
        e = hipMalloc(reinterpret_cast<void **>(&tmp), toff);
    if (e != hipSuccess) {
        if (g)
            (void)hipFree(g);
        svo_set_error("svo_cloud_create: hipMalloc(%zu + %zu) -> %s", keep, toff, hipGetErrorString(e));
        return SVO_ERR_HIP;
    }
    svo_cloud *c = new svo_cloud;
    c->ctx = ctx;
    c->n = n;
    c->block = g;
    c->xyz = reinterpret_cast<float *>(g + o_xyz);
    c->pts = reinterpret_cast<float *>(g + o_pts);
    c->idx = reinterpret_cast<int *>(g + o_idx);
    c->b1 = reinterpret_cast<float *>(g + o_b1);
    c->b2 = reinterpret_cast<float *>(g + o_b2);
    c->b3 = reinterpret_cast<float *>(g + o_b3);
    c->normals = reinterpret_cast<double *>(g + o_nrm);
    c->knn = reinterpret_cast<int *>(g + o_knn);
    c->d_m = reinterpret_cast<int *>(g + o_m);
    uint64_t *k0 = reinterpret_cast<uint64_t *>(tmp + o_k0), *k1 = reinterpret_cast<uint64_t *>(tmp + o_k1);
    int *v1 = reinterpret_cast<int *>(tmp + o_v1);
    unsigned *hist = reinterpret_cast<unsigned *>(tmp + o_hist);
    double *bnd = reinterpret_cast<double *>(tmp + o_bnd);
    hipStream_t st = ctx->stream;
    int rc = SVO_OK;
    auto fail = [&](int code) {
        (void)hipStreamSynchronize(st);
        (void)hipFree(tmp);
        (void)hipFree(g);
        delete c;
        return code;
    };
    // [0] the size, [1] the first non-finite point
    int *head = reinterpret_cast<int *>(ctx->pinned);
    head[0] = n;
    head[1] = 0x7fffffff;
    if (hipMemcpyAsync(c->d_m, head, 8, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(c->xyz, xyz, N * 12, mem == SVO_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, st) !=
            hipSuccess) {
        svo_set_error("svo_cloud_create: the upload failed: %s", hipGetErrorString(hipGetLastError()));
        return fail(SVO_ERR_HIP);
    }
    const dim3 b256(256), g256((n + 255) / 256);
    hipLaunchKernelGGL(cloud_check_kernel, g256, b256, 0, st, c->xyz, n, c->d_m + 1);
    if (hipMemcpyAsync(head + 2, c->d_m + 1, 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) {
        svo_set_error("svo_cloud_create: the finiteness check failed: %s", hipGetErrorString(hipGetLastError()));
        return fail(SVO_ERR_HIP);
    }
    if (head[2] != 0x7fffffff) {
        svo_set_error("svo_cloud_create: point %d has a non-finite coordinate", head[2]);
        return fail(SVO_ERR_ARG);
    }
    hipLaunchKernelGGL(sorg_bounds_kernel, dim3(1), dim3(1024), 0, st, c->xyz, c->d_m, bnd);
    hipLaunchKernelGGL(sorg_key_kernel, g256, b256, 0, st, c->xyz, c->d_m, bnd, n, k0, c->idx);
    if ((rc = radix_sort_pairs(st, k0, c->idx, k1, v1, n, hist)))
        return fail(rc);
    hipLaunchKernelGGL(sorg_gather_kernel, g256, b256, 0, st, c->xyz, c->idx, c->d_m, n, c->pts);
    hipLaunchKernelGGL(sorg_box_kernel, dim3((nb1 + 3) / 4), b256, 0, st, c->pts, c->d_m, 1, nb1, c->b1);
    hipLaunchKernelGGL(sorg_box_kernel, dim3((nb2 + 3) / 4), b256, 0, st, c->b1, c->d_m, 2, nb2, c->b2);
    hipLaunchKernelGGL(sorg_box_kernel, dim3((nb3 + 3) / 4), b256, 0, st, c->b2, c->d_m, 3, nb3, c->b3);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
        svo_set_error("svo_cloud_create: building the index failed: %s", hipGetErrorString(hipGetLastError()));
        return fail(SVO_ERR_HIP);
    }
    (void)hipFree(tmp);
    *out = c;
    return SVO_OK;
}

extern "C" int svo_cloud_destroy(svo_cloud *c)
{
    if (!c)
        return SVO_OK;
    (void)hipStreamSynchronize(c->ctx->stream);
    (void)hipFree(c->block);
    delete c;
    return SVO_OK;
}

extern "C" int svo_cloud_size(const svo_cloud *c) { return c ? c->n : 0; }

extern "C" int svo_cloud_has_normals(const svo_cloud *c) { return c && c->has_normals ? 1 : 0; }

extern "C" int svo_cloud_set_normals(svo_cloud *c, const double *normals, int mem)
{
    SVO_CHECK_ARG(c && normals);
    SVO_CHECK_ARG(mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE);
    SVO_HIP(hipMemcpyAsync(c->normals, normals, (size_t)c->n * 24,
                           mem == SVO_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, c->ctx->stream));
    SVO_HIP(hipStreamSynchronize(c->ctx->stream));
    c->has_normals = true;
    return SVO_OK;
}

extern "C" int svo_cloud_get_normals(svo_cloud *c, double *normals, int mem)
{
    SVO_CHECK_ARG(c && normals);
    SVO_CHECK_ARG(mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE);
    int rc;
    if ((rc = need_normals(c, "svo_cloud_get_normals")))
        return rc;
    SVO_HIP(hipMemcpyAsync(normals, c->normals, (size_t)c->n * 24,
                           mem == SVO_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, c->ctx->stream));
    SVO_HIP(hipStreamSynchronize(c->ctx->stream));
    return SVO_OK;
}

static int check_knn(int k, const char *who)
{
    if (k < 3 || k > 64) {
        svo_set_error("%s: knn %d outside 3 .. 64", who, k);
        return SVO_ERR_ARG;
    }
    return SVO_OK;
}

static void queue_knn(svo_cloud *c, int k)
{
    hipLaunchKernelGGL(cloud_knn_kernel, dim3((c->n + NN_WAVES - 1) / NN_WAVES), dim3(64 * NN_WAVES), 0, c->ctx->stream,
                       cloud_dev(c), k, c->knn);
}

extern "C" int svo_cloud_knn(svo_cloud *c, int k, int *idx_out, int mem)
{
    SVO_CHECK_ARG(c && idx_out);
    SVO_CHECK_ARG(mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE);
    int rc;
    if ((rc = check_knn(k, "svo_cloud_knn")))
        return rc;
    queue_knn(c, k);
    SVO_HIP(hipGetLastError());
    SVO_HIP(hipMemcpyAsync(idx_out, c->knn, (size_t)c->n * k * 4,
                           mem == SVO_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, c->ctx->stream));
    SVO_HIP(hipStreamSynchronize(c->ctx->stream));
    return SVO_OK;
}

extern "C" int svo_cloud_estimate_normals(svo_cloud *c, int knn)
{
    SVO_CHECK_ARG(c);
    int rc;
    if ((rc = check_knn(knn, "svo_cloud_estimate_normals")))
        return rc;
    queue_knn(c, knn);
    hipLaunchKernelGGL(cloud_normals_kernel, dim3((c->n + 255) / 256), dim3(256), 0, c->ctx->stream, cloud_dev(c), knn,
                       c->knn, c->normals);
    SVO_HIP(hipGetLastError());
    c->has_normals = true;
    return SVO_OK;
}

// ---- registration ---------------------------------------------------------------------------------------------------
extern "C" void svo_icp_default_params(svo_icp_params *p)
{
    if (!p)
        return;
    p->max_iteration = 30;
    p->relative_fitness = 1e-6;
    p->relative_rmse = 1e-6;
}

extern "C" int svo_icp_correspondences(svo_ctx *ctx, const float *src_xyz, int n_src, svo_cloud *t, double max_dist,
                                       const double *T16, int *corr_out, double *fitness, double *rmse, int mem)
{
    int rc;
    if ((rc = check_call(ctx, src_xyz, n_src, t, max_dist, T16, mem, "svo_icp_correspondences")))
        return rc;
    IcpWork w;
    const float *src;
    svo_icp_params p;
    svo_icp_default_params(&p);
    if ((rc = icp_work(ctx, n_src, w)) || (rc = stage_source(ctx, w, src_xyz, n_src, mem, &src)))
        return rc;
    hipLaunchKernelGGL(icp_init_kernel, dim3(1), dim3(64), 0, ctx->stream, w.st, mat16(T16), (const IcpState *)nullptr);
    queue_round<MODE_EVAL>(ctx, w, src, n_src, t, max_dist, p, w.st, 1);
    const IcpState *h;
    if ((rc = finish_call(ctx, w, 1, n_src, corr_out, mem, &h)))
        return rc;
    if (fitness)
        *fitness = h->fitness;
    if (rmse)
        *rmse = h->rmse;
    return SVO_OK;
}

extern "C" int svo_icp_normal_equations(svo_ctx *ctx, const float *src_xyz, int n_src, svo_cloud *t, double max_dist,
                                        const double *T16, double *JtJ21, double *Jtr6, int *n_corr, int mem)
{
    int rc;
    if ((rc = check_call(ctx, src_xyz, n_src, t, max_dist, T16, mem, "svo_icp_normal_equations")) ||
        (rc = need_normals(t, "svo_icp_normal_equations")))
        return rc;
    SVO_CHECK_ARG(JtJ21 && Jtr6);
    IcpWork w;
    const float *src;
    svo_icp_params p;
    svo_icp_default_params(&p);
    if ((rc = icp_work(ctx, n_src, w)) || (rc = stage_source(ctx, w, src_xyz, n_src, mem, &src)))
        return rc;
    hipLaunchKernelGGL(icp_init_kernel, dim3(1), dim3(64), 0, ctx->stream, w.st, mat16(T16), (const IcpState *)nullptr);
    queue_round<MODE_ICP>(ctx, w, src, n_src, t, max_dist, p, w.st, 1);
    const IcpState *h;
    if ((rc = finish_call(ctx, w, 1, n_src, nullptr, mem, &h)))
        return rc;
    memcpy(JtJ21, h->JtJ, sizeof(h->JtJ));
    memcpy(Jtr6, h->Jtr, sizeof(h->Jtr));
    if (n_corr)
        *n_corr = h->n_corr;
    return SVO_OK;
}

extern "C" int svo_icp_point_to_plane(svo_ctx *ctx, const float *src_xyz, int n_src, svo_cloud *t, double max_dist,
                                      const double *T_init16, const svo_icp_params *params, double *T_out16,
                                      double *fitness, double *rmse, int *iterations, int *corr_out, int mem)
{
    int rc;
    svo_icp_params p;
    if ((rc = check_call(ctx, src_xyz, n_src, t, max_dist, T_init16, mem, "svo_icp_point_to_plane")) ||
        (rc = check_params(params, p, "svo_icp_point_to_plane")) || (rc = need_normals(t, "svo_icp_point_to_plane")))
        return rc;
    SVO_CHECK_ARG(T_out16);
    IcpWork w;
    const float *src;
    if ((rc = icp_work(ctx, n_src, w)) || (rc = stage_source(ctx, w, src_xyz, n_src, mem, &src)))
        return rc;
    hipLaunchKernelGGL(icp_init_kernel, dim3(1), dim3(64), 0, ctx->stream, w.st, mat16(T_init16),
                       (const IcpState *)nullptr);
    queue_icp(ctx, w, src, n_src, t, max_dist, p, w.st);
    const IcpState *h;
    if ((rc = finish_call(ctx, w, 1, n_src, corr_out, mem, &h)))
        return rc;
    memcpy(T_out16, h->T, sizeof(h->T));
    if (fitness)
        *fitness = h->fitness;
    if (rmse)
        *rmse = h->rmse;
    if (iterations)
        *iterations = h->iterations;
    return SVO_OK;
}

extern "C" int svo_icp_information(svo_ctx *ctx, const float *src_xyz, int n_src, svo_cloud *t, double max_dist,
                                   const double *T16, double *info36, int *n_corr, int mem)
{
    int rc;
    if ((rc = check_call(ctx, src_xyz, n_src, t, max_dist, T16, mem, "svo_icp_information")))
        return rc;
    SVO_CHECK_ARG(info36);
    IcpWork w;
    const float *src;
    svo_icp_params p;
    svo_icp_default_params(&p);
    if ((rc = icp_work(ctx, n_src, w)) || (rc = stage_source(ctx, w, src_xyz, n_src, mem, &src)))
        return rc;
    hipLaunchKernelGGL(icp_init_kernel, dim3(1), dim3(64), 0, ctx->stream, w.st, mat16(T16), (const IcpState *)nullptr);
    queue_round<MODE_INFO>(ctx, w, src, n_src, t, max_dist, p, w.st, 1);
    const IcpState *h;
    if ((rc = finish_call(ctx, w, 1, n_src, nullptr, mem, &h)))
        return rc;
    memcpy(info36, h->info, sizeof(h->info));
    if (n_corr)
        *n_corr = h->n_corr;
    return SVO_OK;
}

extern "C" int svo_icp_pairwise(svo_ctx *ctx, const float *src_xyz, int n_src, svo_cloud *t, double dist_coarse,
                                double dist_fine, const svo_icp_params *params, double *T_out16, double *info36,
                                double *fitness2, double *rmse2, int *iterations2, int *n_corr, int mem)
{
    const double I16[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    int rc;
    svo_icp_params p;
    if ((rc = check_call(ctx, src_xyz, n_src, t, dist_coarse, I16, mem, "svo_icp_pairwise")) ||
        (rc = check_call(ctx, src_xyz, n_src, t, dist_fine, I16, mem, "svo_icp_pairwise")) ||
        (rc = check_params(params, p, "svo_icp_pairwise")) || (rc = need_normals(t, "svo_icp_pairwise")))
        return rc;
    SVO_CHECK_ARG(T_out16 && info36);
    IcpWork w;
    const float *src;
    if ((rc = icp_work(ctx, n_src, w)) || (rc = stage_source(ctx, w, src_xyz, n_src, mem, &src)))
        return rc;
    hipStream_t st = ctx->stream;
    hipLaunchKernelGGL(icp_init_kernel, dim3(1), dim3(64), 0, st, w.st, mat16(I16), (const IcpState *)nullptr);
    queue_icp(ctx, w, src, n_src, t, dist_coarse, p, w.st);
    hipLaunchKernelGGL(icp_init_kernel, dim3(1), dim3(64), 0, st, w.st + 1, mat16(I16), (const IcpState *)w.st);
    queue_icp(ctx, w, src, n_src, t, dist_fine, p, w.st + 1);
    hipLaunchKernelGGL(icp_init_kernel, dim3(1), dim3(64), 0, st, w.st + 2, mat16(I16), (const IcpState *)(w.st + 1));
    queue_round<MODE_INFO>(ctx, w, src, n_src, t, dist_fine, p, w.st + 2, 1);
    const IcpState *h;
    if ((rc = finish_call(ctx, w, 3, n_src, nullptr, mem, &h)))
        return rc;
    memcpy(T_out16, h[1].T, sizeof(h[1].T));
    memcpy(info36, h[2].info, sizeof(h[2].info));
    for (int k = 0; k < 2; k++) {
        if (fitness2)
            fitness2[k] = h[k].fitness;
        if (rmse2)
            rmse2[k] = h[k].rmse;
        if (iterations2)
            iterations2[k] = h[k].iterations;
    }
    if (n_corr)
        *n_corr = h[2].n_corr;
    return SVO_OK;
}

// ---- from Lambda to an edge (host) --------------------------------------------------------------------------------
extern "C" int svo_icp_edge_information(const double *info36, const double *T16, double *info21)
{
    SVO_CHECK_ARG(info36 && T16 && info21);
    const double R[3][3] = {{T16[0], T16[1], T16[2]}, {T16[4], T16[5], T16[6]}, {T16[8], T16[9], T16[10]}};
    const double t[3] = {T16[3], T16[7], T16[11]};
    const double tx[3][3] = {{0, -t[2], t[1]}, {t[2], 0, -t[0]}, {-t[1], t[0], 0}};
    // M^-1 = [0, 2R ; R, 2 [t]x R]: rows (w, v), columns (e_t, e_q)
    double Mi[6][6];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double txr = 0;
            for (int k = 0; k < 3; k++)
                txr += tx[i][k] * R[k][j];
            Mi[i][j] = 0.0;
            Mi[i][3 + j] = 2.0 * R[i][j];
            Mi[3 + i][j] = R[i][j];
            Mi[3 + i][3 + j] = 2.0 * txr;
        }
    double W[6][6];
    for (int i = 0; i < 6; i++)
        for (int j = 0; j < 6; j++) {
            double s = 0;
            for (int k = 0; k < 6; k++)
                s += info36[6 * i + k] * Mi[k][j];
            W[i][j] = s;
        }
    int o = 0;
    for (int i = 0; i < 6; i++)
        for (int j = i; j < 6; j++) {
            double s = 0;
            for (int k = 0; k < 6; k++)
                s += Mi[k][i] * W[k][j];
            info21[o++] = s;
        }
    return SVO_OK;
}

extern "C" int svo_icp_meas7(const double *T16, double *meas7)
{
    SVO_CHECK_ARG(T16 && meas7);
    const double R[9] = {T16[0], T16[1], T16[2], T16[4], T16[5], T16[6], T16[8], T16[9], T16[10]};
    double q[4];
    const double tr = R[0] + R[4] + R[8];
    if (tr > 0) {
        const double s = 2. * sqrt(tr + 1.);
        q[0] = (R[7] - R[5]) / s;
        q[1] = (R[2] - R[6]) / s;
        q[2] = (R[3] - R[1]) / s;
        q[3] = s / 4.;
    } else if (R[0] > R[4] && R[0] > R[8]) {
        const double s = 2. * sqrt(1. + R[0] - R[4] - R[8]);
        q[0] = s / 4.;
        q[1] = (R[1] + R[3]) / s;
        q[2] = (R[2] + R[6]) / s;
        q[3] = (R[7] - R[5]) / s;
    } else if (R[4] > R[8]) {
        const double s = 2. * sqrt(1. + R[4] - R[0] - R[8]);
        q[0] = (R[1] + R[3]) / s;
        q[1] = s / 4.;
        q[2] = (R[5] + R[7]) / s;
        q[3] = (R[2] - R[6]) / s;
    } else {
        const double s = 2. * sqrt(1. + R[8] - R[0] - R[4]);
        q[0] = (R[2] + R[6]) / s;
        q[1] = (R[5] + R[7]) / s;
        q[2] = s / 4.;
        q[3] = (R[3] - R[1]) / s;
    }
    const double nrm = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    const double sgn = q[3] / nrm < 0 ? -1. : 1.;
    meas7[0] = T16[3];
    meas7[1] = T16[7];
    meas7[2] = T16[11];
    for (int k = 0; k < 4; k++)
        meas7[3 + k] = sgn * (q[k] / nrm);
    return SVO_OK;
}
