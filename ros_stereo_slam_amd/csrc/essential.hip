// essential.hip -- essential-matrix RANSAC and pose recovery for gfx950.
//
// Replaces cv::findEssentialMat(p1, p2, K, RANSAC, prob, threshold, mask) and cv::recoverPose(E, p1, p2, K, R, t,
// distanceThresh = 50, mask) of OpenCV 3.2 as the reference's StereoProcess::monocularTriangulate calls them
// (src/StereoCV.cpp:162-163).  Up to SVO_LK_MAX_JOBS independent problems per call (CSR offsets into one point array).
//
//   em_normalise   one thread per point: ((x - cx) / fx, (y - cy) / fy) in double
//   em_iter        one WORKGROUP (four waves) per RANSAC iteration: wave 0 draws the 5-sample (PnP's plain draw, keyed
//                  by (seed, iteration)) and runs the five-point solver (em_solve_wave); all four waves score its up to
//                  ten models with the Sampson error, counts reduced exactly as integers
//   em_replay      one thread per problem replays the SEQUENTIAL loop over the counts (ransac_replay<10>: first-best-
//                  wins, adaptive bound), so the answer is the serial algorithm's whatever the schedule
//   em_final       mask, model, counts
// Three phases (iterations [0, 64), [64, 256), [256, max_iters)); a phase whose problem has already stopped leaves at once.
//
// The five-point solver restates OpenCV 3.2's EMEstimatorCallback::runKernel (five-point.cpp, Nister's method as
// OpenCV writes it): rows [x2 x1, x2 y1, x2, y2 x1, y2 y1, y2, x1, y1, 1]; a 4-dimensional null-space basis
// E = x E0 + y E1 + z E2 + E3; the ten cubic constraints det(E) = 0 and 2 E E^T E - tr(E E^T) E = 0 as a 10 x 20
// matrix in OpenCV's monomial order; A[:, :10]^-1 A[:, 10:]; the 3 x 13 matrix B and det B(z), degree 10; per real
// root, (x, y) from the null vector of B(z) (dropped when its third component is below 1e-10); E at unit Frobenius
// norm.  Where OpenCV uses its SVD and solvePoly, this file chooses (tests/essential_numpy.py restates the choices):
//   null space   Gauss-Jordan with full pivoting (fransac.hip's elimination, one entry per lane), the four null
//                vectors orthonormalised by modified Gram-Schmidt in order;
//   roots        z = zs w with zs = |p0 / p10|^(1/10), then a Sturm sequence in w; isolation by 64-way subdivision
//                (one point per lane; a subinterval where p changes sign holds a root whatever the floating-point
//                counts say), then bracketed Newton per root (one root per lane).  Only real roots exist
//                for it; they come out in ascending z, and the solutions keep that order;
//   polish       four Gauss-Newton steps on the ten cubic constraints in (x, y, z) per root; a solution whose |det E|
//                or trace constraint still exceeds 1e-6 is dropped (a root the arithmetic made up);
//   sign         each E has its entry of largest magnitude (the first, row-major, on a tie) positive.
//
// recoverPose: E = U diag(s) V^T by one-sided Jacobi, the third singular value taken as zero: u1, v1, u2, v2 from the
// two largest, each pair's sign fixed so that v's entry of largest magnitude is positive, u3 = u1 x u2, v3 = v1 x v2
// (det U = det V = +1).  Candidates (U W V^T, u3), (U W^T V^T, u3), (U W V^T, -u3), (U W^T V^T, -u3); a point counts
// for a candidate when the DLT in normalised coordinates (geometry.hip's solver, double) gives Q2 Q3 > 0, z1 < dist
// and 0 < z2 < dist; the input mask ANDs in; the first candidate with the largest count wins (OpenCV's >= order).
#include <cfloat>
#include <cmath>

#include "dlt.hip.h"
#include "ransac_common.hip.h"
#include "svo_internal.h"

using namespace svo;

namespace {

constexpr int MP = 5;        // model points
constexpr int MAXSOL = 10;   // solutions of the five-point solver
constexpr int NW = 4;        // waves per RANSAC workgroup
constexpr int MAX_ITERS = 20000;

// ---- polynomials in (x, y, z) ---------------------------------------------------------------------------------------
// linear form over the variables (x, y, z, 1): L[4]; quadratic form: Q[10], the pair u <= w of variables at qi(u, w);
// cubic: C[20] in OpenCV's monomial order (getCoeffMat's columns):
//   x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x yz^2 yz y z^3 z^2 z 1
__host__ __device__ constexpr int qi(int u, int w)
{
    return u <= w ? u * 4 - u * (u - 1) / 2 + (w - u) : w * 4 - w * (w - 1) / 2 + (u - w);
}
__host__ __device__ constexpr int cub_index(int a, int b, int c)
{
    return a == 3 ? 0 : b == 3 ? 1 : (a == 2 && b == 1) ? 2 : (a == 1 && b == 2) ? 3 : (a == 2 && c == 1) ? 4 : a == 2 ? 5
         : (b == 2 && c == 1) ? 6 : b == 2 ? 7 : (a == 1 && b == 1 && c == 1) ? 8 : (a == 1 && b == 1) ? 9
         : (a == 1 && c == 2) ? 10 : (a == 1 && c == 1) ? 11 : a == 1 ? 12 : (b == 1 && c == 2) ? 13
         : (b == 1 && c == 1) ? 14 : b == 1 ? 15 : c == 3 ? 16 : c == 2 ? 17 : c == 1 ? 18 : 19;
}
__host__ __device__ constexpr int var_cub_index(int u, int w, int v)
{
    return cub_index((u == 0) + (w == 0) + (v == 0), (u == 1) + (w == 1) + (v == 1), (u == 2) + (w == 2) + (v == 2));
}

// q += s * a * b
__device__ __forceinline__ void acc_ll(double (&q)[10], const double (&a)[4], const double (&b)[4], double s)
{
#pragma unroll
    for (int u = 0; u < 4; u++)
#pragma unroll
        for (int w = 0; w < 4; w++)
            q[qi(u, w)] += s * a[u] * b[w];
}
// c += s * q * l
__device__ __forceinline__ void acc_ql(double (&c)[20], const double (&q)[10], const double (&l)[4], double s)
{
#pragma unroll
    for (int u = 0; u < 4; u++)
#pragma unroll
        for (int w = u; w < 4; w++)
#pragma unroll
            for (int v = 0; v < 4; v++)
                c[var_cub_index(u, w, v)] += s * q[qi(u, w)] * l[v];
}
// entry m (row-major) of E(x, y, z) as a linear form
__device__ __forceinline__ void load_L(const double *Eb, int m, double (&L)[4])
{
#pragma unroll
    for (int v = 0; v < 4; v++)
        L[v] = Eb[v * 9 + m];
}

// out[0 .. DA + DB] = a[0 .. DA] * b[0 .. DB] (ascending powers)
template <int DA, int DB> __device__ __forceinline__ void polymul(const double *a, const double *b, double *out)
{
#pragma unroll
    for (int k = 0; k <= DA + DB; k++)
        out[k] = 0;
#pragma unroll
    for (int i = 0; i <= DA; i++)
#pragma unroll
        for (int j = 0; j <= DB; j++)
            out[i + j] += a[i] * b[j];
}

// LDS of one five-point solve
struct EmLds {
    double A[45];          // 5 x 9 system after elimination
    double Eb[36];         // null-space basis E0 .. E3, row-major 3 x 3 each
    double Q[90];          // E E^T, nine quadratics
    double M[200];         // 10 x 20 coefficient matrix
    double C[100];         // A[:, :10]^-1 A[:, 10:]
    double B[39];          // 3 x 13
    double st[11 * 11];    // Sturm sequence, ascending powers, each scaled to max |coefficient| 1
    double ia[16], ib[16]; // work stack of intervals
    double ra[MAXSOL], rb[MAXSOL], root[MAXSOL];
    double sol[MAXSOL * 9];
    int sdeg[11], va[16], vb[16];
    double zs;             // z = zs * w: the Sturm chain is in w
    int perm[9];
    int ns, nstack, nr, nsol;
};

// monomial m (OpenCV's order) of (x, y, z) and its gradient
__device__ __forceinline__ void mono_grad(double x, double y, double z, double (&m)[20], double (&g)[20][3])
{
    const double px[4] = {1., x, x * x, x * x * x}, py[4] = {1., y, y * y, y * y * y}, pz[4] = {1., z, z * z, z * z * z};
#pragma unroll
    for (int a = 0; a <= 3; a++)
#pragma unroll
        for (int b = 0; a + b <= 3; b++)
#pragma unroll
            for (int c = 0; a + b + c <= 3; c++) {
                const int k = cub_index(a, b, c);
                m[k] = px[a] * py[b] * pz[c];
                g[k][0] = a ? a * px[a - 1] * py[b] * pz[c] : 0.;
                g[k][1] = b ? b * px[a] * py[b - 1] * pz[c] : 0.;
                g[k][2] = c ? c * px[a] * py[b] * pz[c - 1] : 0.;
            }
}

// |det E| and max |2 E E^T E - tr(E E^T) E| of a unit-norm E
__device__ __forceinline__ double e_residual(const double (&E)[9])
{
    double EEt[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++)
            EEt[3 * i + j] = E[3 * i] * E[3 * j] + E[3 * i + 1] * E[3 * j + 1] + E[3 * i + 2] * E[3 * j + 2];
    const double tr = EEt[0] + EEt[4] + EEt[8];
    double r = fabs(E[0] * (E[4] * E[8] - E[5] * E[7]) - E[1] * (E[3] * E[8] - E[5] * E[6]) + E[2] * (E[3] * E[7] - E[4] * E[6]));
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const double v = 2. * (EEt[3 * i] * E[j] + EEt[3 * i + 1] * E[3 + j] + EEt[3 * i + 2] * E[6 + j]) - tr * E[3 * i + j];
            r = fmax(r, fabs(v));
        }
    return r;
}

__device__ __forceinline__ int sgn(double v) { return v > 0 ? 1 : (v < 0 ? -1 : 0); }

__device__ int sturm_count(const EmLds &S, double t)
{
    int V = 0, prev = 0;
    for (int k = 0; k < S.ns; k++) {
        const double *c = S.st + k * 11;
        const int d = S.sdeg[k];
        double r = c[d];
        for (int j = d - 1; j >= 0; j--)
            r = r * t + c[j];
        const int s = sgn(r);
        if (s != 0) {
            V += (prev != 0 && s != prev) ? 1 : 0;
            prev = s;
        }
    }
    return V;
}
// the first polynomial of the chain (p in w) at t
__device__ __forceinline__ double poly_eval(const EmLds &S, double t)
{
    const int d = S.sdeg[0];
    double r = S.st[d];
    for (int j = d - 1; j >= 0; j--)
        r = r * t + S.st[j];
    return r;
}
// at -inf (neg) / +inf: the signs of the leading coefficients
__device__ int sturm_count_inf(const EmLds &S, bool neg)
{
    int V = 0, prev = 0;
    for (int k = 0; k < S.ns; k++) {
        const int d = S.sdeg[k];
        int s = sgn(S.st[k * 11 + d]);
        if (neg && (d & 1))
            s = -s;
        if (s != 0) {
            V += (prev != 0 && s != prev) ? 1 : 0;
            prev = s;
        }
    }
    return V;
}

// lane 0: the Sturm sequence of p[0..10] into S (S.ns = 0: no real root)
__device__ void sturm_build(EmLds &S, const double (&p)[11])
{
    S.ns = 0;
    double mx = 0;
    for (int d = 0; d <= 10; d++)
        mx = fmax(mx, fabs(p[d]));
    if (!(mx > 0) || !isfinite(mx))
        return;
    int deg = 10;
    while (deg > 0 && fabs(p[deg]) <= 1e-14 * mx)
        deg--;
    if (deg == 0)
        return;
    for (int d = 0; d <= deg; d++)
        S.st[d] = p[d] / mx;
    S.sdeg[0] = deg;
    double m1 = 0;
    for (int d = 1; d <= deg; d++)
        m1 = fmax(m1, fabs(d * S.st[d]));
    for (int d = 1; d <= deg; d++)
        S.st[11 + d - 1] = d * S.st[d] / m1;
    S.sdeg[1] = deg - 1;
    int ns = 2;
    while (ns < 11 && S.sdeg[ns - 1] > 0) {
        double *r = S.st + ns * 11;
        const double *a = S.st + (ns - 2) * 11, *b = S.st + (ns - 1) * 11;
        const int da = S.sdeg[ns - 2], db = S.sdeg[ns - 1];
        for (int d = 0; d <= da; d++)
            r[d] = a[d];
        for (int d = da; d >= db; d--) {
            const double f = r[d] / b[db];
            for (int j = 0; j <= db; j++)
                r[d - db + j] -= f * b[j];
            r[d] = 0;
        }
        double m = 0;
        for (int d = 0; d < db; d++)
            m = fmax(m, fabs(r[d]));
        if (!(m > 1e-13))
            break;  // the remainder vanishes: the chain ends at the gcd
        int dr = db - 1;
        while (dr > 0 && fabs(r[dr]) <= 1e-14 * m)
            dr--;
        for (int d = 0; d <= dr; d++)
            r[d] = -r[d] / m;
        S.sdeg[ns] = dr;
        ns++;
    }
    S.ns = ns;
}

// One five-point solve by one WAVE: the sample idx of the normalised points q1 / q2; the solutions (row-major,
// ascending z) into S.sol; returns their number (wave-uniform).
__device__ int em_solve_wave(const double2 *__restrict__ q1, const double2 *__restrict__ q2, const int (&idx)[MP],
                             EmLds &S, int lane)
{
    // ---- 5 x 9 system, one entry per lane; Gauss-Jordan with full pivoting (as fr_solve_wave) ----
    const bool valid = lane < MP * 9;
    const int li = valid ? lane / 9 : MP, lj = valid ? lane - 9 * li : 0;
    double a = 0;
    {
        int my = idx[0];
#pragma unroll
        for (int i = 1; i < MP; i++)
            my = li == i ? idx[i] : my;
        const double2 u = q1[my], w = q2[my];
        const double x1 = u.x, y1 = u.y, x2 = w.x, y2 = w.y;
        const double row[9] = {x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, 1.};
#pragma unroll
        for (int j = 0; j < 9; j++)
            a = lj == j ? row[j] : a;
        if (!valid)
            a = 0;
    }
    int permv = lane;
#pragma unroll 1
    for (int k = 0; k < MP; k++) {
        const double v = (valid && li >= k && lj >= k) ? fabs(a) : -1.;
        const double best = wave_max(v);
        if (!(best >= 1e-12))
            return 0;  // degenerate sample (wave-uniform)
        const int pl = __ffsll((unsigned long long)__ballot(v == best)) - 1;
        const int pr = pl / 9, pc = pl - 9 * pr;
        if (pr != k) {
            const int src = li == k ? pr * 9 + lj : (li == pr ? k * 9 + lj : lane);
            a = __shfl(a, src, 64);
        }
        if (pc != k) {
            const int src = lj == k ? li * 9 + pc : (lj == pc ? li * 9 + k : lane);
            a = __shfl(a, valid ? src : lane, 64);
            const int psrc = lane == k ? pc : (lane == pc ? k : lane);
            permv = __shfl(permv, psrc, 64);
        }
        const double piv = __shfl(a, k * 9 + k, 64);
        if (li == k)
            a /= piv;
        const double rowk = __shfl(a, k * 9 + lj, 64);
        const double f = __shfl(a, valid ? li * 9 + k : lane, 64);
        if (valid && li != k && f != 0)
            a -= f * rowk;
    }
    if (valid)
        S.A[lane] = a;
    if (lane < 9)
        S.perm[lane] = permv;
    wave_lds_fence();
    // ---- null-space basis: free column 5 + f -> E_f; modified Gram-Schmidt in order ----
    if (lane == 0) {
        for (int f = 0; f < 4; f++) {
            double *e = S.Eb + f * 9;
            for (int i = 0; i < 9; i++)
                e[i] = 0;
            for (int k = 0; k < MP; k++)
                e[S.perm[k]] = -S.A[k * 9 + 5 + f];
            e[S.perm[5 + f]] = 1;
            for (int g = 0; g < f; g++) {
                const double *h = S.Eb + g * 9;
                double d = 0;
                for (int i = 0; i < 9; i++)
                    d += h[i] * e[i];
                for (int i = 0; i < 9; i++)
                    e[i] -= d * h[i];
            }
            double nn = 0;
            for (int i = 0; i < 9; i++)
                nn += e[i] * e[i];
            nn = sqrt(nn);
            for (int i = 0; i < 9; i++)
                e[i] /= nn;
        }
    }
    wave_lds_fence();
    // ---- E E^T: lane 3 i + j holds entry (i, j) ----
    if (lane < 9) {
        const int i = lane / 3, j = lane - 3 * i;
        double q[10];
#pragma unroll
        for (int p = 0; p < 10; p++)
            q[p] = 0;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            double La[4], Lb[4];
            load_L(S.Eb, 3 * i + k, La);
            load_L(S.Eb, 3 * j + k, Lb);
            acc_ll(q, La, Lb, 1.);
        }
#pragma unroll
        for (int p = 0; p < 10; p++)
            S.Q[lane * 10 + p] = q[p];
    }
    wave_lds_fence();
    // ---- the ten cubic constraints: lanes 0..8 the entries of 2 E E^T E - tr(E E^T) E, lane 9 det(E) ----
    if (lane < 10) {
        double c[20];
#pragma unroll
        for (int m = 0; m < 20; m++)
            c[m] = 0;
        if (lane < 9) {
            const int i = lane / 3, j = lane - 3 * i;
            double q[10], L[4];
#pragma unroll
            for (int k = 0; k < 3; k++) {
#pragma unroll
                for (int p = 0; p < 10; p++)
                    q[p] = S.Q[(3 * i + k) * 10 + p];
                load_L(S.Eb, 3 * k + j, L);
                acc_ql(c, q, L, 2.);
            }
#pragma unroll
            for (int p = 0; p < 10; p++)
                q[p] = S.Q[0 * 10 + p] + S.Q[4 * 10 + p] + S.Q[8 * 10 + p];
            load_L(S.Eb, 3 * i + j, L);
            acc_ql(c, q, L, -1.);
        } else {
            double L[9][4];
#pragma unroll
            for (int m = 0; m < 9; m++)
                load_L(S.Eb, m, L[m]);
            double m0[10], m1[10], m2[10];
#pragma unroll
            for (int p = 0; p < 10; p++)
                m0[p] = m1[p] = m2[p] = 0;
            acc_ll(m0, L[4], L[8], 1.);
            acc_ll(m0, L[5], L[7], -1.);
            acc_ll(m1, L[3], L[8], 1.);
            acc_ll(m1, L[5], L[6], -1.);
            acc_ll(m2, L[3], L[7], 1.);
            acc_ll(m2, L[4], L[6], -1.);
            acc_ql(c, m0, L[0], 1.);
            acc_ql(c, m1, L[1], -1.);
            acc_ql(c, m2, L[2], 1.);
        }
#pragma unroll
        for (int m = 0; m < 20; m++)
            S.M[lane * 20 + m] = c[m];
    }
    wave_lds_fence();
    // ---- A[:, :10]^-1 A[:, 10:]: Gauss-Jordan with partial pivoting, lane j holds column j ----
    {
        double col[10];
#pragma unroll
        for (int r = 0; r < 10; r++)
            col[r] = lane < 20 ? S.M[r * 20 + lane] : 0.;
#pragma unroll
        for (int k = 0; k < 10; k++) {
            double ck[10];
#pragma unroll
            for (int r = 0; r < 10; r++)
                ck[r] = __shfl(col[r], k, 64);
            int p = k;
            double best = fabs(ck[k]);
#pragma unroll
            for (int r = k + 1; r < 10; r++)
                if (fabs(ck[r]) > best) {
                    best = fabs(ck[r]);
                    p = r;
                }
            if (!(best > 0) || !isfinite(best))
                return 0;  // wave-uniform
            double rowp = col[k], cp = ck[k];
#pragma unroll
            for (int r = k + 1; r < 10; r++)
                if (r == p) {
                    rowp = col[r];
                    cp = ck[r];
                    col[r] = col[k];
                    ck[r] = ck[k];
                }
            col[k] = rowp / cp;
#pragma unroll
            for (int r = 0; r < 10; r++)
                if (r != k)
                    col[r] -= ck[r] * col[k];
        }
        if (lane >= 10 && lane < 20)
#pragma unroll
            for (int r = 0; r < 10; r++)
                S.C[r * 10 + lane - 10] = col[r];
    }
    wave_lds_fence();
    // ---- B (3 x 13), det B(z) (degree 10), its Sturm sequence ----
    if (lane == 0) {
        for (int i = 0; i < 3; i++) {
            const double *a1 = S.C + (2 * i + 4) * 10, *a2 = S.C + (2 * i + 5) * 10;
            double r1[13], r2[13];
            for (int m = 0; m < 13; m++)
                r1[m] = r2[m] = 0;
            for (int m = 0; m < 3; m++) {
                r1[1 + m] = a1[m];
                r1[5 + m] = a1[3 + m];
                r2[m] = a2[m];
                r2[4 + m] = a2[3 + m];
            }
            for (int m = 0; m < 4; m++) {
                r1[9 + m] = a1[6 + m];
                r2[8 + m] = a2[6 + m];
            }
            for (int m = 0; m < 13; m++)
                S.B[i * 13 + m] = r1[m] - r2[m];
        }
        // b0[j], b1[j]: entries (j, 0), (j, 1) of B(z), cubics; b2[j]: entry (j, 2), a quartic; ascending powers
        double b0[3][4], b1[3][4], b2[3][5];
        for (int j = 0; j < 3; j++) {
            const double *br = S.B + j * 13;
            for (int m = 0; m < 4; m++) {
                b0[j][m] = br[3 - m];
                b1[j][m] = br[7 - m];
            }
            for (int m = 0; m < 5; m++)
                b2[j][m] = br[12 - m];
        }
        double t7a[8], t7b[8], t6a[7], t6b[7], m0[8], m1[8], m2[7], p[11], tmp[11];
        polymul<3, 4>(b1[1], b2[2], t7a);
        polymul<4, 3>(b2[1], b1[2], t7b);
        for (int k = 0; k < 8; k++)
            m0[k] = t7a[k] - t7b[k];
        polymul<3, 4>(b0[1], b2[2], t7a);
        polymul<4, 3>(b2[1], b0[2], t7b);
        for (int k = 0; k < 8; k++)
            m1[k] = t7a[k] - t7b[k];
        polymul<3, 3>(b0[1], b1[2], t6a);
        polymul<3, 3>(b1[1], b0[2], t6b);
        for (int k = 0; k < 7; k++)
            m2[k] = t6a[k] - t6b[k];
        polymul<3, 7>(b0[0], m0, p);
        polymul<3, 7>(b1[0], m1, tmp);
        for (int k = 0; k < 11; k++)
            p[k] -= tmp[k];
        polymul<4, 6>(b2[0], m2, tmp);
        for (int k = 0; k < 11; k++)
            p[k] += tmp[k];
        // z = zs w with zs = |p0 / p10|^(1/10): roots near magnitude one, coefficients balanced for the Sturm chain
        double zs = 1.;
        if (p[0] != 0 && p[10] != 0 && isfinite(p[0] / p[10]))
            zs = pow(fabs(p[0] / p[10]), 0.1);
        zs = zs > 0 && isfinite(zs) ? zs : 1.;
        S.zs = zs;
        double zk = 1.;
        for (int k = 0; k < 11; k++) {
            p[k] *= zk;
            zk *= zs;
        }
        sturm_build(S, p);
        S.nr = 0;
        S.nstack = 0;
        if (S.ns > 0) {
            // Fujiwara's bound on the magnitude of the roots
            const int d = S.sdeg[0];
            const double *c = S.st;
            double R = 0;
            for (int k = 1; k <= d; k++) {
                double r = fabs(c[d - k] / c[d]);
                if (k == d)
                    r *= 0.5;
                R = fmax(R, pow(r, 1. / k));
            }
            R = 2. * R * 1.0625 + 1e-300;
            S.ia[0] = -R;
            S.ib[0] = R;
            S.va[0] = sturm_count_inf(S, true);
            S.vb[0] = sturm_count_inf(S, false);
            S.nstack = 1;
        }
    }
    wave_lds_fence();
    // ---- isolation: 64-way subdivision of the interval on top of the stack, one Sturm count per lane ----
#pragma unroll 1
    for (int round = 0; round < 256; round++) {
        const int nst = S.nstack;
        if (nst == 0)
            break;
        const double a0 = S.ia[nst - 1], b0 = S.ib[nst - 1];
        const int va0 = S.va[nst - 1], vb0 = S.vb[nst - 1];
        wave_lds_fence();
        const int cnt = va0 - vb0;
        int nstack = nst - 1;
        if (cnt == 1 || (cnt > 1 && !(b0 - a0 > 1e-15 * fmax(fabs(a0), fabs(b0))))) {
            if (lane == 0 && S.nr < MAXSOL) {  // isolated (or a cluster narrower than the arithmetic resolves: once)
                S.ra[S.nr] = cnt == 1 ? a0 : 0.5 * (a0 + b0);
                S.rb[S.nr] = cnt == 1 ? b0 : 0.5 * (a0 + b0);
                S.nr++;
            }
        } else if (cnt > 1) {
            // a subinterval holds Vl - V roots by the counts; a sign change of p in it proves at least one, which the
            // counts of a floating-point chain can miss -- such an interval is taken as isolated
            const double t = lane == 63 ? b0 : a0 + (b0 - a0) * ((double)(lane + 1) * (1. / 64));
            int V = sturm_count(S, t);
            V = lane == 63 ? vb0 : V;
            const int sp = sgn(poly_eval(S, t)), sa = sgn(poly_eval(S, a0));
            // every lane takes part in the shuffles (a lane that skipped one would hand its neighbour a zero)
            const double t_up = __shfl(t, (lane + 63) & 63, 64);
            const int V_up = __shfl(V, (lane + 63) & 63, 64), sp_up = __shfl(sp, (lane + 63) & 63, 64);
            const double tl = lane == 0 ? a0 : t_up;
            const int Vl = lane == 0 ? va0 : V_up;
            const int spl = lane == 0 ? sa : sp_up;
            const int c = Vl - V >= 1 ? Vl - V : (spl * sp < 0 ? 1 : 0);
            const bool push = c >= 1;
            const unsigned long long bal = __ballot(push);
            const int pos = nstack + __popcll(bal & ((1ull << lane) - 1ull));
            if (push && pos < 16) {
                S.ia[pos] = tl;
                S.ib[pos] = t;
                S.va[pos] = Vl;
                S.vb[pos] = Vl - c;
            }
            nstack += __popcll(bal);
            nstack = nstack > 16 ? 16 : nstack;
        }
        if (lane == 0)
            S.nstack = nstack;
        wave_lds_fence();
    }
    // ---- ascending order, then one root per lane: bracketed Newton on the first Sturm polynomial ----
    if (lane == 0)
        for (int i = 1; i < S.nr; i++)
            for (int j = i; j > 0 && S.ra[j] < S.ra[j - 1]; j--) {
                double t = S.ra[j];
                S.ra[j] = S.ra[j - 1];
                S.ra[j - 1] = t;
                t = S.rb[j];
                S.rb[j] = S.rb[j - 1];
                S.rb[j - 1] = t;
            }
    wave_lds_fence();
    const int nr = S.nr;
    if (lane < nr) {
        double lo = S.ra[lane], hi = S.rb[lane];
        const double *c = S.st;
        const int d = S.sdeg[0];
        auto eval = [&](double x, double &fp) {
            double f = c[d], g = 0;
            for (int j = d - 1; j >= 0; j--) {
                g = g * x + f;
                f = f * x + c[j];
            }
            fp = g;
            return f;
        };
        double x = 0.5 * (lo + hi), fp;
        if (hi > lo) {
            const int slo = sgn(eval(lo, fp));
            for (int it = 0; it < 200; it++) {
                const double f = eval(x, fp);
                if (f == 0)
                    break;
                if (sgn(f) == slo)
                    lo = x;
                else
                    hi = x;
                double xn = x - f / fp;
                if (!(xn > lo && xn < hi))
                    xn = 0.5 * (lo + hi);
                const bool done = fabs(xn - x) <= 4. * DBL_EPSILON * fabs(x) ||
                                  !(hi - lo > 2. * DBL_EPSILON * fmax(fabs(lo), fabs(hi)));
                x = xn;
                if (done)
                    break;
            }
        }
        S.root[lane] = x * S.zs;
    }
    wave_lds_fence();
    // ---- per root: B(z), its null vector, (x, y), E ----
    bool keep = false;
    double E[9];
    if (lane < nr) {
        const double z1 = S.root[lane], z2 = z1 * z1, z3 = z2 * z1, z4 = z3 * z1;
        double bz[9];
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const double *br = S.B + j * 13;
            bz[j * 3 + 0] = br[0] * z3 + br[1] * z2 + br[2] * z1 + br[3];
            bz[j * 3 + 1] = br[4] * z3 + br[5] * z2 + br[6] * z1 + br[7];
            bz[j * 3 + 2] = br[8] * z4 + br[9] * z3 + br[10] * z2 + br[11] * z1 + br[12];
        }
        // the null vector of a rank-2 3 x 3 matrix: the longest cross product of two of its rows
        double v[3] = {0, 0, 0}, vn = 0;
#pragma unroll
        for (int pr = 0; pr < 3; pr++) {
            const int r0 = pr == 2 ? 1 : 0, r1 = pr == 0 ? 1 : 2;
            const double *ra = bz + 3 * r0, *rb = bz + 3 * r1;
            const double cx = ra[1] * rb[2] - ra[2] * rb[1], cy = ra[2] * rb[0] - ra[0] * rb[2],
                         cz = ra[0] * rb[1] - ra[1] * rb[0];
            const double nn = cx * cx + cy * cy + cz * cz;
            if (nn > vn) {
                vn = nn;
                v[0] = cx, v[1] = cy, v[2] = cz;
            }
        }
        vn = sqrt(vn);
        if (vn > 0 && isfinite(vn)) {
#pragma unroll
            for (int k = 0; k < 3; k++)
                v[k] /= vn;
            if (fabs(v[2]) >= 1e-10) {
                double x = v[0] / v[2], y = v[1] / v[2], z = z1;
                // four Gauss-Newton steps on the ten cubic constraints (the 10 x 20 matrix) in (x, y, z)
                for (int step = 0; step < 4; step++) {
                    double m[20], g[20][3], JtJ[6] = {0, 0, 0, 0, 0, 0}, Jtf[3] = {0, 0, 0};
                    mono_grad(x, y, z, m, g);
                    for (int r = 0; r < 10; r++) {
                        const double *row = S.M + r * 20;
                        double f = 0, j0 = 0, j1 = 0, j2 = 0;
#pragma unroll
                        for (int k = 0; k < 20; k++) {
                            f += row[k] * m[k];
                            j0 += row[k] * g[k][0];
                            j1 += row[k] * g[k][1];
                            j2 += row[k] * g[k][2];
                        }
                        JtJ[0] += j0 * j0, JtJ[1] += j0 * j1, JtJ[2] += j0 * j2;
                        JtJ[3] += j1 * j1, JtJ[4] += j1 * j2, JtJ[5] += j2 * j2;
                        Jtf[0] += j0 * f, Jtf[1] += j1 * f, Jtf[2] += j2 * f;
                    }
                    // (J^T J) d = -J^T f by Cramer's rule
                    const double a = JtJ[0], b = JtJ[1], c = JtJ[2], d = JtJ[3], e = JtJ[4], h = JtJ[5];
                    const double c0 = d * h - e * e, c1 = c * e - b * h, c2 = b * e - c * d;
                    const double det = a * c0 + b * c1 + c * c2;
                    if (!(fabs(det) > 0) || !isfinite(det))
                        break;
                    const double i11 = a * h - c * c, i12 = b * c - a * e, i22 = a * d - b * b;
                    const double dx = -(c0 * Jtf[0] + c1 * Jtf[1] + c2 * Jtf[2]) / det;
                    const double dy = -(c1 * Jtf[0] + i11 * Jtf[1] + i12 * Jtf[2]) / det;
                    const double dz = -(c2 * Jtf[0] + i12 * Jtf[1] + i22 * Jtf[2]) / det;
                    if (!isfinite(dx) || !isfinite(dy) || !isfinite(dz))
                        break;
                    x += dx, y += dy, z += dz;
                }
                double nrm = 0;
#pragma unroll
                for (int i = 0; i < 9; i++) {
                    E[i] = S.Eb[i] * x + S.Eb[9 + i] * y + S.Eb[18 + i] * z + S.Eb[27 + i];
                    nrm += E[i] * E[i];
                }
                nrm = sqrt(nrm);
                if (nrm > 0 && isfinite(nrm)) {
                    int im = 0;
#pragma unroll
                    for (int i = 0; i < 9; i++) {
                        E[i] /= nrm;
                        im = fabs(E[i]) > fabs(E[im]) ? i : im;
                    }
                    double sg = 1.;
#pragma unroll
                    for (int i = 0; i < 9; i++)
                        sg = i == im ? (E[i] < 0 ? -1. : 1.) : sg;
#pragma unroll
                    for (int i = 0; i < 9; i++)
                        E[i] *= sg;
                    keep = e_residual(E) <= 1e-6;  // a root of det B(z) that the arithmetic made up: no essential matrix
                }
            }
        }
    }
    const unsigned long long bal = __ballot(keep);
    if (keep) {
        const int pos = __popcll(bal & ((1ull << lane) - 1ull));
#pragma unroll
        for (int i = 0; i < 9; i++)
            S.sol[pos * 9 + i] = E[i];
    }
    wave_lds_fence();
    return __popcll(bal);
}

// cv EMEstimatorCallback::computeError (normalised points, double arithmetic, float result)
__device__ __forceinline__ float em_error(const double (&E)[9], double x1, double y1, double x2, double y2)
{
    const double ex0 = E[0] * x1 + E[1] * y1 + E[2];
    const double ex1 = E[3] * x1 + E[4] * y1 + E[5];
    const double ex2 = E[6] * x1 + E[7] * y1 + E[8];
    const double et0 = E[0] * x2 + E[3] * y2 + E[6];
    const double et1 = E[1] * x2 + E[4] * y2 + E[7];
    const double d = x2 * ex0 + y2 * ex1 + ex2;
    return (float)(d * d / (ex0 * ex0 + ex1 * ex1 + et0 * et0 + et1 * et1));
}

struct EmJob {
    const float *p1, *p2;   // pixels, n pairs
    double2 *q1, *q2;       // normalised (workspace)
    int n;
    double fx, fy, cx, cy;
    float thr;              // (threshold / ((fx + fy) / 2))^2
    RansacState *st;
    double *Em;             // max_iters x 10 x 9
    int *nmodels, *counts;  // max_iters, max_iters x 10
    uint8_t *mask;
    double *E_out;          // 10 x 9
    int *nmod_out, *count_out, *iters_out;
};
struct EmBatch {
    EmJob j[SVO_LK_MAX_JOBS];
};
static_assert(sizeof(EmBatch) + 64 <= 4096, "kernel arguments are limited to 4 KB");

__global__ __launch_bounds__(256) void em_normalise_kernel(EmBatch b)
{
    const EmJob &job = b.j[blockIdx.y];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= job.n)
        return;
    job.q1[i] = make_double2(((double)job.p1[2 * i] - job.cx) / job.fx, ((double)job.p1[2 * i + 1] - job.cy) / job.fy);
    job.q2[i] = make_double2(((double)job.p2[2 * i] - job.cx) / job.fx, ((double)job.p2[2 * i + 1] - job.cy) / job.fy);
}

// iterations [it0, min(it1, max_iters)) of every problem, a workgroup per iteration (see the file header)
__global__ __launch_bounds__(256) void em_iter_kernel(EmBatch b, uint64_t seed, int max_iters, int it0, int it1)
{
    svo_chain_priority();
    const EmJob &job = b.j[blockIdx.y];
    const int n = job.n;
    if (n < MP || (n == MP && it0 > 0))
        return;
    int lim = it1 < max_iters ? it1 : max_iters;
    if (n == MP)
        lim = 1;  // findEssentialMat on exactly five pairs: the solver once, on the pairs as they stand
    if (it0 > 0) {
        const RansacState s = *job.st;  // written by the previous phase's replay
        if (s.done)
            return;
        lim = lim < s.niters ? lim : s.niters;
    }
    __shared__ EmLds S;
    __shared__ int s_cnt[NW][MAXSOL];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double2 *__restrict__ q1 = job.q1, *__restrict__ q2 = job.q2;
    for (int it = it0 + (int)blockIdx.x; it < lim; it += gridDim.x) {
        if (wave == 0) {
            int idx[MP] = {0, 1, 2, 3, 4};
            uint32_t draw = 0;
            const bool ok = n == MP || draw_distinct(seed, it, n, draw, idx);
            const int nm = ok ? em_solve_wave(q1, q2, idx, S, lane) : -1;
            if (lane == 0) {
                S.nsol = nm;
                job.nmodels[it] = nm;
            }
            for (int e = lane; e < (nm > 0 ? nm : 0) * 9; e += 64)
                job.Em[(size_t)it * MAXSOL * 9 + e] = S.sol[e];
        }
        __syncthreads();
        const int nm = S.nsol;
        if (n > MP && nm > 0) {
            for (int k = 0; k < nm; k++) {
                double E[9];
#pragma unroll
                for (int i = 0; i < 9; i++)
                    E[i] = S.sol[k * 9 + i];
                int c = 0;
                for (int i = threadIdx.x; i < n; i += 256) {
                    const double2 u = q1[i], w = q2[i];
                    c += em_error(E, u.x, u.y, w.x, w.y) <= job.thr ? 1 : 0;
                }
                c = wave_sum_dpp(c);
                if (lane == 0)
                    s_cnt[wave][k] = c;
            }
        }
        __syncthreads();
        if (threadIdx.x == 0 && n > MP)
            for (int k = 0; k < nm; k++)
                job.counts[it * MAXSOL + k] = s_cnt[0][k] + s_cnt[1][k] + s_cnt[2][k] + s_cnt[3][k];
        __syncthreads();  // S / s_cnt are rewritten by the next iteration of this workgroup
    }
}

__global__ void em_replay_kernel(EmBatch b, double confidence, int max_iters, int it_end, int first)
{
    const EmJob &job = b.j[blockIdx.x];
    if (threadIdx.x != 0)
        return;
    if (job.n <= MP) {  // no loop: fewer than five pairs (no model) or exactly five (the solver once)
        RansacState r;
        r.niters = 0, r.next_iter = 0, r.best_iter = -1, r.best_model = 0, r.best_count = 0, r.done = 1, r.iters_run = 0;
        r.pad = 0;
        *job.st = r;
        return;
    }
    *job.st = ransac_replay<MAXSOL>(job.st, first, it_end < max_iters ? it_end : max_iters, max_iters, job.n, confidence,
                                    job.nmodels, job.counts, MP);
}

__global__ __launch_bounds__(256) void em_final_kernel(EmBatch b)
{
    const EmJob &job = b.j[blockIdx.y];
    const int n = job.n;
    const RansacState s = *job.st;
    int nm = 0, count = 0;
    const double *Eb = job.Em;
    if (n == MP) {
        nm = job.nmodels[0] > 0 ? job.nmodels[0] : 0;
        count = nm > 0 ? MP : 0;
    } else if (n > MP && s.best_iter >= 0 && s.best_count > 0) {
        nm = 1;
        count = s.best_count;
        Eb = job.Em + ((size_t)s.best_iter * MAXSOL + s.best_model) * 9;
    }
    double E[9];
#pragma unroll
    for (int i = 0; i < 9; i++)
        E[i] = nm > 0 ? Eb[i] : 0.;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        bool in = false;
        if (n == MP)
            in = nm > 0;
        else if (nm > 0) {
            const double2 u = job.q1[i], w = job.q2[i];
            in = em_error(E, u.x, u.y, w.x, w.y) <= job.thr;
        }
        job.mask[i] = in ? 1 : 0;
    }
    if (blockIdx.x == 0) {
        if (job.E_out)
            for (int e = threadIdx.x; e < MAXSOL * 9; e += blockDim.x)
                job.E_out[e] = e < nm * 9 ? Eb[e] : 0.;
        if (threadIdx.x == 0) {
            if (job.nmod_out)
                *job.nmod_out = nm;
            if (job.count_out)
                *job.count_out = count;
            if (job.iters_out)
                *job.iters_out = n > MP ? s.iters_run : 0;
        }
    }
}

__global__ __launch_bounds__(64) void em_5pt_kernel(const double *x1n, const double *x2n, double *E_out, int *nsol)
{
    __shared__ EmLds S;
    const int lane = threadIdx.x;
    const int s = blockIdx.x;
    const double2 *q1 = reinterpret_cast<const double2 *>(x1n) + (size_t)s * MP;
    const double2 *q2 = reinterpret_cast<const double2 *>(x2n) + (size_t)s * MP;
    const int idx[MP] = {0, 1, 2, 3, 4};
    const int nm = em_solve_wave(q1, q2, idx, S, lane);
    for (int e = lane; e < MAXSOL * 9; e += 64)
        E_out[(size_t)s * MAXSOL * 9 + e] = e < nm * 9 ? S.sol[e] : 0.;
    if (lane == 0)
        nsol[s] = nm;
}

// ---- recoverPose --------------------------------------------------------------------------------------------------
// E = U diag(s) V^T (one-sided Jacobi on E's columns) -> R1 = U W V^T, R2 = U W^T V^T, t = u3 (the file header's
// sign rules).  Host and device.
__host__ __device__ void em_decompose(const double *E, double *R1, double *R2, double *t)
{
    double A[3][3], V[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            A[i][j] = E[3 * i + j];
            V[i][j] = i == j ? 1. : 0.;
        }
    for (int sweep = 0; sweep < 40; sweep++) {
        bool rotated = false;
        for (int p = 0; p < 2; p++)
            for (int q = p + 1; q < 3; q++) {
                double al = 0, be = 0, ga = 0;
                for (int i = 0; i < 3; i++) {
                    al += A[i][p] * A[i][p];
                    be += A[i][q] * A[i][q];
                    ga += A[i][p] * A[i][q];
                }
                if (ga == 0 || fabs(ga) <= DBL_EPSILON * sqrt(al * be))
                    continue;
                rotated = true;
                const double zeta = (be - al) / (2. * ga);
                const double tt = (zeta >= 0 ? 1. : -1.) / (fabs(zeta) + sqrt(1. + zeta * zeta));
                const double c = 1. / sqrt(1. + tt * tt), s = c * tt;
                for (int i = 0; i < 3; i++) {
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
    double sv[3];
    for (int j = 0; j < 3; j++)
        sv[j] = sqrt(A[0][j] * A[0][j] + A[1][j] * A[1][j] + A[2][j] * A[2][j]);
    int o[3] = {0, 1, 2};
    for (int i = 1; i < 3; i++)
        for (int j = i; j > 0 && sv[o[j]] > sv[o[j - 1]]; j--) {
            const int x = o[j];
            o[j] = o[j - 1];
            o[j - 1] = x;
        }
    double u[3][3], v[3][3];  // u[k], v[k]: the k-th singular vectors
    for (int k = 0; k < 2; k++) {
        const int c = o[k];
        int im = 0;
        for (int i = 0; i < 3; i++) {
            v[k][i] = V[i][c];
            u[k][i] = sv[c] > 0 ? A[i][c] / sv[c] : 0.;
        }
        for (int i = 1; i < 3; i++)
            im = fabs(v[k][i]) > fabs(v[k][im]) ? i : im;
        if (v[k][im] < 0)
            for (int i = 0; i < 3; i++) {
                v[k][i] = -v[k][i];
                u[k][i] = -u[k][i];
            }
    }
    u[2][0] = u[0][1] * u[1][2] - u[0][2] * u[1][1];
    u[2][1] = u[0][2] * u[1][0] - u[0][0] * u[1][2];
    u[2][2] = u[0][0] * u[1][1] - u[0][1] * u[1][0];
    v[2][0] = v[0][1] * v[1][2] - v[0][2] * v[1][1];
    v[2][1] = v[0][2] * v[1][0] - v[0][0] * v[1][2];
    v[2][2] = v[0][0] * v[1][1] - v[0][1] * v[1][0];
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) {
            const double a = u[0][i] * v[1][j], bb = u[1][i] * v[0][j], c = u[2][i] * v[2][j];
            R1[3 * i + j] = a - bb + c;
            R2[3 * i + j] = -a + bb + c;
        }
        t[i] = u[2][i];
    }
}

struct RpJob {
    const float *p1, *p2;
    int n;
    double fx, fy, cx, cy;
    const double *E;
    uint8_t *mask;   // in / out, or null
    uint8_t *good4;  // workspace: 4 x n candidate masks
    int *cnt4;       // workspace: 4 counts (zeroed)
    double *R, *t;
    int *good;
};
struct RpBatch {
    RpJob j[SVO_LK_MAX_JOBS];
};
static_assert(sizeof(RpBatch) + 64 <= 4096, "kernel arguments are limited to 4 KB");

// a wave per candidate, a workgroup per 64 points; counts by integer atomics (exact, order-free)
__global__ __launch_bounds__(256) void rp_count_kernel(RpBatch b, double dist)
{
    const RpJob &job = b.j[blockIdx.y];
    if ((int)blockIdx.x * 64 >= job.n)
        return;
    __shared__ double sR[2][9], sT[3];
    if (threadIdx.x == 0)
        em_decompose(job.E, sR[0], sR[1], sT);
    __syncthreads();
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    double P[12];
    const double ts = w < 2 ? 1. : -1.;
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++)
            P[4 * r + c] = sR[w & 1][3 * r + c];
        P[4 * r + 3] = ts * sT[r];
    }
    const int i = blockIdx.x * 64 + lane;
    bool g = false;
    if (i < job.n) {
        const double x1 = ((double)job.p1[2 * i] - job.cx) / job.fx, y1 = ((double)job.p1[2 * i + 1] - job.cy) / job.fy;
        const double x2 = ((double)job.p2[2 * i] - job.cx) / job.fx, y2 = ((double)job.p2[2 * i + 1] - job.cy) / job.fy;
        g = rp_point_good(P, x1, y1, x2, y2, dist) && (!job.mask || job.mask[i] != 0);
        job.good4[(size_t)w * job.n + i] = g ? 1 : 0;
    }
    const int c = __popcll(__ballot(g));
    if (lane == 0 && c)
        atomicAdd(job.cnt4 + w, c);
}

__global__ __launch_bounds__(256) void rp_pick_kernel(RpBatch b)
{
    const RpJob &job = b.j[blockIdx.y];
    const int g1 = job.cnt4[0], g2 = job.cnt4[1], g3 = job.cnt4[2], g4 = job.cnt4[3];
    int pick;
    if (g1 >= g2 && g1 >= g3 && g1 >= g4)
        pick = 0;
    else if (g2 >= g1 && g2 >= g3 && g2 >= g4)
        pick = 1;
    else if (g3 >= g1 && g3 >= g2 && g3 >= g4)
        pick = 2;
    else
        pick = 3;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (job.mask && i < job.n)
        job.mask[i] = job.good4[(size_t)pick * job.n + i];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        double R1[9], R2[9], t[3];
        em_decompose(job.E, R1, R2, t);
        for (int k = 0; k < 9; k++)
            job.R[k] = (pick & 1) ? R2[k] : R1[k];
        for (int k = 0; k < 3; k++)
            job.t[k] = pick < 2 ? t[k] : -t[k];
        if (job.good)
            *job.good = pick == 0 ? g1 : pick == 1 ? g2 : pick == 2 ? g3 : g4;
    }
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// the problems' offsets and intrinsics (host memory): SVO_ERR_ARG when malformed, else the end of the last problem
int check_problems(const int *offsets, int nprob, const double *K4, int *total)
{
    SVO_CHECK_ARG(offsets && K4 && nprob >= 1 && nprob <= SVO_LK_MAX_JOBS);
    SVO_CHECK_ARG(offsets[0] >= 0);
    for (int k = 0; k < nprob; k++) {
        SVO_CHECK_ARG(offsets[k + 1] >= offsets[k]);
        SVO_CHECK_ARG(K4[4 * k] != 0 && K4[4 * k + 1] != 0 && std::isfinite(K4[4 * k]) && std::isfinite(K4[4 * k + 1]) &&
                      std::isfinite(K4[4 * k + 2]) && std::isfinite(K4[4 * k + 3]));
    }
    *total = offsets[nprob];
    return SVO_OK;
}

}  // namespace

extern "C" int svo_decompose_essential(const double *E9, double *R1, double *R2, double *t)
{
    SVO_CHECK_ARG(E9 && R1 && R2 && t);
    for (int k = 0; k < 9; k++)
        SVO_CHECK_ARG(std::isfinite(E9[k]));
    em_decompose(E9, R1, R2, t);
    return SVO_OK;
}

extern "C" int svo_essential_5pt(svo_ctx *ctx, const double *x1n, const double *x2n, int nsamples, double *E_out, int *nsol,
                                 int mem)
{
    SVO_CHECK_ARG(ctx && nsamples >= 0 && (mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE));
    if (nsamples == 0)
        return SVO_OK;
    SVO_CHECK_ARG(x1n && x2n && E_out && nsol);
    const size_t in_b = (size_t)nsamples * MP * 2 * sizeof(double), e_b = (size_t)nsamples * MAXSOL * 9 * sizeof(double);
    const size_t n_b = (size_t)nsamples * sizeof(int);
    ScopedKernelTime tm(ctx, SVO_K_FRANSAC);
    if (mem == SVO_MEM_DEVICE) {
        hipLaunchKernelGGL(em_5pt_kernel, dim3(nsamples), dim3(64), 0, ctx->stream, x1n, x2n, E_out, nsol);
        SVO_HIP(hipGetLastError());
        return SVO_OK;
    }
    int rc;
    if ((rc = ctx->s_a.ensure(in_b)) || (rc = ctx->s_b.ensure(in_b)) || (rc = ctx->s_c.ensure(e_b)) ||
        (rc = ctx->s_d.ensure(n_b)))
        return rc;
    SVO_HIP(hipMemcpyAsync(ctx->s_a.p, x1n, in_b, hipMemcpyHostToDevice, ctx->stream));
    SVO_HIP(hipMemcpyAsync(ctx->s_b.p, x2n, in_b, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(em_5pt_kernel, dim3(nsamples), dim3(64), 0, ctx->stream, ctx->s_a.as<double>(), ctx->s_b.as<double>(),
                       ctx->s_c.as<double>(), ctx->s_d.as<int>());
    SVO_HIP(hipGetLastError());
    SVO_HIP(hipMemcpyAsync(E_out, ctx->s_c.p, e_b, hipMemcpyDeviceToHost, ctx->stream));
    SVO_HIP(hipMemcpyAsync(nsol, ctx->s_d.p, n_b, hipMemcpyDeviceToHost, ctx->stream));
    SVO_HIP(hipStreamSynchronize(ctx->stream));
    return SVO_OK;
}

extern "C" int svo_find_essential(svo_ctx *ctx, const float *p1, const float *p2, const int *offsets, int nprob,
                                  const double *K4, double threshold, double confidence, int max_iters, uint64_t seed,
                                  uint8_t *mask, double *E_out, int *nmodels, int *inlier_count, int *iters_run, int mem)
{
    SVO_CHECK_ARG(ctx && (mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE));
    int total = 0, rc;
    if ((rc = check_problems(offsets, nprob, K4, &total)))
        return rc;
    SVO_CHECK_ARG(threshold > 0 && std::isfinite(threshold) && confidence > 0 && confidence < 1);
    SVO_CHECK_ARG(max_iters >= 1 && max_iters <= MAX_ITERS);
    SVO_CHECK_ARG(total == 0 || (p1 && p2 && mask));
    const int base = offsets[0];
    // workspace: normalised points, then per problem the models / model counts / inlier counts / state
    const size_t q_b = align256((size_t)(total + 1) * sizeof(double2));
    const size_t em_b = align256((size_t)max_iters * MAXSOL * 9 * sizeof(double));
    const size_t ct_b = align256((size_t)max_iters * (MAXSOL + 1) * sizeof(int) + sizeof(RansacState));
    const size_t ws = 2 * q_b + (size_t)nprob * (em_b + ct_b);
    // host mode: the staged inputs and outputs behind the workspace
    const size_t pin_b = align256((size_t)(total + 1) * 2 * sizeof(float)), mask_b = align256((size_t)total + 1);
    const size_t out_b = align256((size_t)nprob * (MAXSOL * 9 * sizeof(double) + 3 * sizeof(int)));
    const size_t stage = mem == SVO_MEM_HOST ? 2 * pin_b + mask_b + out_b : 0;
    if ((rc = ctx->ess.ensure(ws + stage)))
        return rc;
    char *w = ctx->ess.as<char>();
    const float *d1 = p1, *d2 = p2;
    uint8_t *dmask = mask;
    double *dE = E_out;
    int *dnm = nmodels, *dcnt = inlier_count, *dit = iters_run;
    if (mem == SVO_MEM_HOST) {
        char *stg = w + ws;
        float *s1 = reinterpret_cast<float *>(stg), *s2 = reinterpret_cast<float *>(stg + pin_b);
        if (total > base) {
            SVO_HIP(hipMemcpyAsync(s1 + 2 * base, p1 + 2 * base, (size_t)(total - base) * 8, hipMemcpyHostToDevice, ctx->stream));
            SVO_HIP(hipMemcpyAsync(s2 + 2 * base, p2 + 2 * base, (size_t)(total - base) * 8, hipMemcpyHostToDevice, ctx->stream));
        }
        d1 = s1, d2 = s2;
        dmask = reinterpret_cast<uint8_t *>(stg + 2 * pin_b);
        dE = reinterpret_cast<double *>(stg + 2 * pin_b + mask_b);
        dnm = reinterpret_cast<int *>(dE + (size_t)nprob * MAXSOL * 9);
        dcnt = dnm + nprob;
        dit = dcnt + nprob;
    }
    EmBatch b;
    int nmax = 0;
    for (int k = 0; k < nprob; k++) {
        EmJob &j = b.j[k];
        const int o = offsets[k], n = offsets[k + 1] - offsets[k];
        j.p1 = d1 ? d1 + 2 * (size_t)o : nullptr;
        j.p2 = d2 ? d2 + 2 * (size_t)o : nullptr;
        j.q1 = reinterpret_cast<double2 *>(w) + o;
        j.q2 = reinterpret_cast<double2 *>(w + q_b) + o;
        j.n = n;
        j.fx = K4[4 * k], j.fy = K4[4 * k + 1], j.cx = K4[4 * k + 2], j.cy = K4[4 * k + 3];
        const double thr_n = threshold / ((j.fx + j.fy) / 2);
        j.thr = (float)(thr_n * thr_n);
        char *pw = w + 2 * q_b + (size_t)k * (em_b + ct_b);
        j.Em = reinterpret_cast<double *>(pw);
        j.st = reinterpret_cast<RansacState *>(pw + em_b);
        j.nmodels = reinterpret_cast<int *>(j.st + 1);
        j.counts = j.nmodels + max_iters;
        j.mask = dmask ? dmask + o : nullptr;
        j.E_out = dE ? dE + (size_t)k * MAXSOL * 9 : nullptr;
        j.nmod_out = dnm ? dnm + k : nullptr;
        j.count_out = dcnt ? dcnt + k : nullptr;
        j.iters_out = dit ? dit + k : nullptr;
        nmax = n > nmax ? n : nmax;
    }
    for (int k = nprob; k < SVO_LK_MAX_JOBS; k++)
        b.j[k] = b.j[0];
    {
        ScopedKernelTime tm(ctx, SVO_K_FRANSAC);
        if (nmax > 0)
            hipLaunchKernelGGL(em_normalise_kernel, dim3((nmax + 255) / 256, nprob), dim3(256), 0, ctx->stream, b);
        const int bounds[3] = {0, 64, 256};
        for (int ph = 0; ph < 3; ph++) {
            const int it0 = bounds[ph];
            const int it1 = ph == 2 ? max_iters : (bounds[ph + 1] < max_iters ? bounds[ph + 1] : max_iters);
            if (it0 >= it1)
                break;
            const int groups = it1 - it0 < 256 ? it1 - it0 : 256;
            hipLaunchKernelGGL(em_iter_kernel, dim3(groups, nprob), dim3(256), 0, ctx->stream, b, seed, max_iters, it0, it1);
            hipLaunchKernelGGL(em_replay_kernel, dim3(nprob), dim3(64), 0, ctx->stream, b, confidence, max_iters, it1,
                               ph == 0 ? 1 : 0);
        }
        hipLaunchKernelGGL(em_final_kernel, dim3(nmax > 0 ? (nmax + 255) / 256 : 1, nprob), dim3(256), 0, ctx->stream, b);
        SVO_HIP(hipGetLastError());
    }
    if (mem == SVO_MEM_DEVICE)
        return SVO_OK;
    if (total > base)
        SVO_HIP(hipMemcpyAsync(mask + base, dmask + base, (size_t)(total - base), hipMemcpyDeviceToHost, ctx->stream));
    if (E_out)
        SVO_HIP(hipMemcpyAsync(E_out, dE, (size_t)nprob * MAXSOL * 9 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (nmodels)
        SVO_HIP(hipMemcpyAsync(nmodels, dnm, (size_t)nprob * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    if (inlier_count)
        SVO_HIP(hipMemcpyAsync(inlier_count, dcnt, (size_t)nprob * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    if (iters_run)
        SVO_HIP(hipMemcpyAsync(iters_run, dit, (size_t)nprob * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    SVO_HIP(hipStreamSynchronize(ctx->stream));
    return SVO_OK;
}

extern "C" int svo_recover_pose(svo_ctx *ctx, const double *E9, const float *p1, const float *p2, const int *offsets,
                                int nprob, const double *K4, double distance_thresh, uint8_t *mask_inout, double *R9,
                                double *t3, int *good, int mem)
{
    SVO_CHECK_ARG(ctx && (mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE));
    int total = 0, rc;
    if ((rc = check_problems(offsets, nprob, K4, &total)))
        return rc;
    SVO_CHECK_ARG(E9 && R9 && t3 && distance_thresh > 0);
    SVO_CHECK_ARG(total == 0 || (p1 && p2));
    const int base = offsets[0];
    const size_t g_b = align256((size_t)4 * (total + 1)), c_b = align256((size_t)nprob * 4 * sizeof(int));
    const size_t pin_b = align256((size_t)(total + 1) * 2 * sizeof(float)), mask_b = align256((size_t)total + 1);
    const size_t eo_b = align256((size_t)nprob * (9 + 9 + 3) * sizeof(double) + (size_t)nprob * sizeof(int));
    const size_t stage = mem == SVO_MEM_HOST ? 2 * pin_b + mask_b + eo_b : 0;
    if ((rc = ctx->ess.ensure(g_b + c_b + stage)))
        return rc;
    char *w = ctx->ess.as<char>();
    uint8_t *good4 = reinterpret_cast<uint8_t *>(w);
    int *cnt = reinterpret_cast<int *>(w + g_b);
    const float *d1 = p1, *d2 = p2;
    const double *dE = E9;
    uint8_t *dmask = mask_inout;
    double *dR = R9, *dt = t3;
    int *dgood = good;
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
        double *eo = reinterpret_cast<double *>(stg + 2 * pin_b + mask_b);
        SVO_HIP(hipMemcpyAsync(eo, E9, (size_t)nprob * 9 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        dE = eo;
        dR = eo + (size_t)nprob * 9;
        dt = dR + (size_t)nprob * 9;
        dgood = reinterpret_cast<int *>(dt + (size_t)nprob * 3);
    }
    SVO_HIP(hipMemsetAsync(cnt, 0, (size_t)nprob * 4 * sizeof(int), ctx->stream));
    RpBatch b;
    int nmax = 0;
    for (int k = 0; k < nprob; k++) {
        RpJob &j = b.j[k];
        const int o = offsets[k], n = offsets[k + 1] - offsets[k];
        j.p1 = d1 ? d1 + 2 * (size_t)o : nullptr;
        j.p2 = d2 ? d2 + 2 * (size_t)o : nullptr;
        j.n = n;
        j.fx = K4[4 * k], j.fy = K4[4 * k + 1], j.cx = K4[4 * k + 2], j.cy = K4[4 * k + 3];
        j.E = dE + 9 * (size_t)k;
        j.mask = dmask ? dmask + o : nullptr;
        j.good4 = good4 + 4 * (size_t)o;
        j.cnt4 = cnt + 4 * k;
        j.R = dR + 9 * (size_t)k;
        j.t = dt + 3 * (size_t)k;
        j.good = dgood ? dgood + k : nullptr;
        nmax = n > nmax ? n : nmax;
    }
    for (int k = nprob; k < SVO_LK_MAX_JOBS; k++)
        b.j[k] = b.j[0];
    {
        ScopedKernelTime tm(ctx, SVO_K_TRIANGULATE);
        if (nmax > 0)
            hipLaunchKernelGGL(rp_count_kernel, dim3((nmax + 63) / 64, nprob), dim3(256), 0, ctx->stream, b, distance_thresh);
        hipLaunchKernelGGL(rp_pick_kernel, dim3(nmax > 0 ? (nmax + 255) / 256 : 1, nprob), dim3(256), 0, ctx->stream, b);
        SVO_HIP(hipGetLastError());
    }
    if (mem == SVO_MEM_DEVICE)
        return SVO_OK;
    if (mask_inout && total > base)
        SVO_HIP(hipMemcpyAsync(mask_inout + base, dmask + base, (size_t)(total - base), hipMemcpyDeviceToHost, ctx->stream));
    SVO_HIP(hipMemcpyAsync(R9, dR, (size_t)nprob * 9 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    SVO_HIP(hipMemcpyAsync(t3, dt, (size_t)nprob * 3 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (good)
        SVO_HIP(hipMemcpyAsync(good, dgood, (size_t)nprob * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    SVO_HIP(hipStreamSynchronize(ctx->stream));
    return SVO_OK;
}
