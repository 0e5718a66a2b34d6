// rectify_plan.hip.h -- the host decisions of rectify.hip with nothing of the HIP runtime in them: the camera model, the
// fixed-point conversion and the undistortion of one point (shared with the kernels, so what runs on the device is what is
// checked here), Rodrigues, Bouguet's stereoRectify, the inverse the map kernel starts from, the argument and capacity refusals
// and the launch geometry.  rectify.hip includes it; so does tests/cpp/rectify_plan_check.cpp, a stand-alone program that runs
// it under the address and undefined-behaviour sanitizers.  The definition is tests/rectify_numpy.py's (points N1 - N15).
#pragma once

#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/svo.h"

#if defined(__HIPCC__)
#define RECT_PLAN_HD __host__ __device__
#else
#define RECT_PLAN_HD
#endif

namespace rectify_plan {

constexpr int MAX_DIM = 32767;              // the int16 map: a width or height above it is refused
constexpr long long MAX_PIXELS = 1ll << 30; // pixels per call (map pixels, and source pixels) over all images
constexpr int MAX_IMAGES = 16;              // images of a batch, pairs of a pair call
constexpr int MAX_POINTS = 1 << 24;         // points of one svo_undistort_points call
constexpr int QUAD = 4;                     // output pixels a thread of the remap takes
constexpr int BLOCK_X = 64, BLOCK_Y = 4;    // threads of a remap workgroup: quads along a row x rows

// N1: k1 k2 p1 p2 k3 k4 k5 k6
struct Coeffs {
    double k[8];
};
inline bool nd_ok(int nD) { return nD == 0 || nD == 4 || nD == 5 || nD == 8; }
inline Coeffs coeffs(const double *D, int nD)
{
    Coeffs c;
    for (int i = 0; i < 8; i++)
        c.k[i] = i < nD ? D[i] : 0.0;
    return c;
}
inline bool finite_all(const double *p, int n)
{
    for (int i = 0; i < n; i++)
        if (!std::isfinite(p[i]))
            return false;
    return true;
}

// N2
RECT_PLAN_HD inline double kr(double r2, const Coeffs &c)
{
    return (1 + ((c.k[4] * r2 + c.k[1]) * r2 + c.k[0]) * r2) / (1 + ((c.k[7] * r2 + c.k[6]) * r2 + c.k[5]) * r2);
}
RECT_PLAN_HD inline void tangential(double x, double y, double r2, const Coeffs &c, double *dx, double *dy)
{
    const double a1 = (2 * x) * y;
    *dx = c.k[2] * a1 + c.k[3] * (r2 + (2 * x) * x);
    *dy = c.k[2] * (r2 + (2 * y) * y) + c.k[3] * a1;
}
// K4: fx fy cx cy
RECT_PLAN_HD inline void distort(double x, double y, const double *K4, const Coeffs &c, double *u, double *v)
{
    const double r2 = x * x + y * y, s = kr(r2, c);
    double dx, dy;
    tangential(x, y, r2, c, &dx, &dy);
    *u = K4[0] * (x * s + dx) + K4[2];
    *v = K4[1] * (y * s + dy) + K4[3];
}

// N11: rint(v * 32) as an int the way x86's conversion gives it
RECT_PLAN_HD inline int fix5(double v)
{
    const double r = rint(v * 32);
    return (r >= -2147483648.0 && r < 2147483648.0) ? (int)r : INT_MIN;  // false for a NaN
}
RECT_PLAN_HD inline int sat16(int v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }
// N11, N12: the map words of a source coordinate; the shift of a negative int is arithmetic (floor), the mask its residue
RECT_PLAN_HD inline void map_words(double u, double v, short *x, short *y, unsigned short *frac)
{
    const int iu = fix5(u), iv = fix5(v);
    *x = (short)sat16(iu >> 5);
    *y = (short)sat16(iv >> 5);
    *frac = (unsigned short)((iv & 31) * 32 + (iu & 31));
}

// N10 + N2: output pixel (j, i) -> its unrounded source coordinate
struct MapModel {
    double iR[9];
    double K4[4];
    Coeffs c;
};
RECT_PLAN_HD inline void map_pixel(const MapModel &m, int j, int i, double *u, double *v)
{
    const double X = j * m.iR[0] + (i * m.iR[1] + m.iR[2]);
    const double Y = j * m.iR[3] + (i * m.iR[4] + m.iR[5]);
    const double W = j * m.iR[6] + (i * m.iR[7] + m.iR[8]);
    distort(X / W, Y / W, m.K4, m.c, u, v);
}

// N13: one point; R9 / P4 (P[0][0] P[1][1] P[0][2] P[1][2]) optional through has_R / has_P
struct UndistortModel {
    double K4[4];
    Coeffs c;
    double R[9], P4[4];
    int has_R, has_P;
};
RECT_PLAN_HD inline void undistort_one(const UndistortModel &m, double u, double v, double *ox, double *oy)
{
    const double x0 = (u - m.K4[2]) / m.K4[0], y0 = (v - m.K4[3]) / m.K4[1];
    double x = x0, y = y0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int it = 0; it < 5; it++) {
        const double r2 = x * x + y * y, icd = 1.0 / kr(r2, m.c);
        double dx, dy;
        tangential(x, y, r2, m.c, &dx, &dy);
        x = (x0 - dx) * icd;
        y = (y0 - dy) * icd;
    }
    if (m.has_R) {
        const double X = (m.R[0] * x + m.R[1] * y) + m.R[2];
        const double Y = (m.R[3] * x + m.R[4] * y) + m.R[5];
        const double W = (m.R[6] * x + m.R[7] * y) + m.R[8];
        x = X / W;
        y = Y / W;
    }
    if (m.has_P) {
        x = x * m.P4[0] + m.P4[2];
        y = y * m.P4[1] + m.P4[3];
    }
    *ox = x;
    *oy = y;
}

inline void mat3(const double *A, const double *B, double *out)
{
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++)
            out[3 * r + c] = (A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c]) + A[3 * r + 2] * B[6 + c];
}
inline void mat3v(const double *A, const double *v, double *out)
{
    for (int r = 0; r < 3; r++)
        out[r] = (A[3 * r] * v[0] + A[3 * r + 1] * v[1]) + A[3 * r + 2] * v[2];
}
// N9; false when the determinant is zero or not finite
inline bool inv3(const double *m, double *out)
{
    const double c00 = m[4] * m[8] - m[5] * m[7], c01 = m[5] * m[6] - m[3] * m[8], c02 = m[3] * m[7] - m[4] * m[6];
    const double det = (m[0] * c00 + m[1] * c01) + m[2] * c02;
    if (!(det != 0.0) || !std::isfinite(det))
        return false;
    const double adj[9] = {c00, m[2] * m[7] - m[1] * m[8], m[1] * m[5] - m[2] * m[4],
                           c01, m[0] * m[8] - m[2] * m[6], m[2] * m[3] - m[0] * m[5],
                           c02, m[1] * m[6] - m[0] * m[7], m[0] * m[4] - m[1] * m[3]};
    for (int i = 0; i < 9; i++)
        out[i] = adj[i] / det;
    return true;
}

// N3, N4
inline void rodrigues_matrix(const double *v, double *R)
{
    const double theta = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    for (int i = 0; i < 9; i++)
        R[i] = i % 4 == 0 ? 1.0 : 0.0;
    if (theta < 2.220446049250313e-16)
        return;
    const double c = std::cos(theta), s = std::sin(theta), c1 = 1 - c;
    const double r[3] = {v[0] / theta, v[1] / theta, v[2] / theta};
    const double rx[9] = {0, -r[2], r[1], r[2], 0, -r[0], -r[1], r[0], 0};
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++)
            R[3 * a + b] = (c * (a == b ? 1.0 : 0.0) + c1 * (r[a] * r[b])) + s * rx[3 * a + b];
}
inline void rodrigues_vector(const double *R, double *v)
{
    double r[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
    const double s = std::sqrt((r[0] * r[0] + r[1] * r[1] + r[2] * r[2]) * 0.25);
    double c = (R[0] + R[4] + R[8] - 1) * 0.5;
    c = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);
    const double theta = std::acos(c);
    if (s < 1e-5) {
        if (c > 0) {
            v[0] = v[1] = v[2] = 0.0;
            return;
        }
        auto half = [](double d) { const double t = (d + 1) * 0.5; return std::sqrt(t > 0.0 ? t : 0.0); };
        r[0] = half(R[0]);
        r[1] = half(R[4]) * (R[1] < 0 ? -1.0 : 1.0);
        r[2] = half(R[8]) * (R[2] < 0 ? -1.0 : 1.0);
        if (std::fabs(r[0]) < std::fabs(r[1]) && std::fabs(r[0]) < std::fabs(r[2]) && (R[5] > 0) != (r[1] * r[2] > 0))
            r[2] = -r[2];
        const double f = theta / std::sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
        for (int i = 0; i < 3; i++)
            v[i] = r[i] * f;
        return;
    }
    const double f = (1 / (2 * s)) * theta;
    for (int i = 0; i < 3; i++)
        v[i] = r[i] * f;
}

inline UndistortModel undistort_model(const double *K9, const double *D, int nD, const double *R9, const double *P12)
{
    UndistortModel m;
    m.K4[0] = K9[0], m.K4[1] = K9[4], m.K4[2] = K9[2], m.K4[3] = K9[5];
    m.c = coeffs(D, nD);
    m.has_R = R9 != nullptr;
    m.has_P = P12 != nullptr;
    for (int i = 0; i < 9; i++)
        m.R[i] = R9 ? R9[i] : (i % 4 == 0 ? 1.0 : 0.0);
    m.P4[0] = P12 ? P12[0] : 1.0, m.P4[1] = P12 ? P12[5] : 1.0, m.P4[2] = P12 ? P12[2] : 0.0, m.P4[3] = P12 ? P12[6] : 0.0;
    return m;
}

// what the camera arguments shared by every entry point are refused for; 0, or the reason
inline const char *check_camera(const double *K9, const double *D, int nD)
{
    if (!K9)
        return "K must not be null";
    if (!nd_ok(nD))
        return "D must hold 0, 4, 5 or 8 coefficients (thin-prism and tilt terms are not built)";
    if (nD > 0 && !D)
        return "D must not be null when nD is not 0";
    if (!finite_all(K9, 9) || (nD > 0 && !finite_all(D, nD)))
        return "K and D must be finite";
    if (K9[0] == 0.0 || K9[4] == 0.0)
        return "the focal lengths must not be zero";
    return nullptr;
}

// svo_undistort_points_host: float points in, DOUBLE points out
inline const char *undistort_points_host(const float *xy, int n, const double *K9, const double *D, int nD, const double *R9,
                                         const double *P12, double *out_xy)
{
    if (n < 0)
        return "n must not be negative";
    if (const char *why = check_camera(K9, D, nD))
        return why;
    if ((R9 && !finite_all(R9, 9)) || (P12 && !finite_all(P12, 12)))
        return "R and P must be finite";
    if (n > 0 && (!xy || !out_xy))
        return "xy and out_xy must not be null when n is not 0";
    const UndistortModel m = undistort_model(K9, D, nD, R9, P12);
    for (size_t i = 0; i < (size_t)n; i++)  // 2 i passes 2^31 for n above 2^30
        undistort_one(m, (double)xy[2 * i], (double)xy[2 * i + 1], &out_xy[2 * i], &out_xy[2 * i + 1]);
    return nullptr;
}

constexpr int CALIB_ZERO_DISPARITY = 1024;

// svo_stereo_rectify (N5 - N8): 0, or the reason with nothing written
inline const char *stereo_rectify(const double *K1, const double *D1, int nD1, const double *K2, const double *D2, int nD2, int w,
                                  int h, const double *R, const double *T, int flags, double alpha, int new_w, int new_h,
                                  double *R1, double *R2, double *P1, double *P2, double *Q)
{
    if (!R || !T || !R1 || !R2 || !P1 || !P2 || !Q)
        return "R, T and the five outputs must not be null";
    if (const char *why = check_camera(K1, D1, nD1))
        return why;
    if (const char *why = check_camera(K2, D2, nD2))
        return why;
    if (w <= 0 || h <= 0 || new_w < 0 || new_h < 0 || (new_w == 0) != (new_h == 0))
        return "the image size must be positive, the new size positive or 0 x 0";
    if (!(alpha == -1.0))
        return "alpha must be -1: the free scaling parameter and the valid ROIs are not built";
    if (!finite_all(R, 9) || !finite_all(T, 3))
        return "R and T must be finite";
    if (T[0] == 0.0 && T[1] == 0.0 && T[2] == 0.0)
        return "T must not be zero";
    const double *Ks[2] = {K1, K2};
    const Coeffs cs[2] = {coeffs(D1, nD1), coeffs(D2, nD2)};
    // 1.
    double om[3], r_r[9], r_rT[9], t[3];
    rodrigues_vector(R, om);
    for (int i = 0; i < 3; i++)
        om[i] = om[i] * -0.5;
    rodrigues_matrix(om, r_r);
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++)
            r_rT[3 * a + b] = r_r[3 * b + a];
    mat3v(r_r, T, t);
    // 2.
    const int idx = std::fabs(t[0]) > std::fabs(t[1]) ? 0 : 1;
    const double c = t[idx], nt = std::sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
    double uu[3] = {0, 0, 0};
    uu[idx] = c > 0 ? 1.0 : -1.0;
    // 3.
    double ww[3] = {t[1] * uu[2] - t[2] * uu[1], t[2] * uu[0] - t[0] * uu[2], t[0] * uu[1] - t[1] * uu[0]};
    const double nw = std::sqrt(ww[0] * ww[0] + ww[1] * ww[1] + ww[2] * ww[2]);
    if (nw > 0) {
        const double f = std::acos(std::fabs(c) / nt) / nw;
        for (int i = 0; i < 3; i++)
            ww[i] = ww[i] * f;
    }
    double wR[9], r1[9], r2[9];
    rodrigues_matrix(ww, wR);
    // 4.
    mat3(wR, r_rT, r1);
    mat3(wR, r_r, r2);
    mat3v(r2, T, t);
    if (!(t[idx] != 0.0) || !std::isfinite(t[idx]))
        return "R and T give no baseline";
    // 5.
    double fc_new = HUGE_VAL;
    for (int k = 0; k < 2; k++) {
        double fc = Ks[k][4 * (idx ^ 1)];
        if (cs[k].k[0] < 0)
            fc = fc * (1 + cs[k].k[0] * ((double)w * w + (double)h * h) / (4 * fc * fc));
        fc_new = fc < fc_new ? fc : fc_new;
    }
    // 6. (N6: the corners are float points after the undistortion and after the projection)
    const float corners[8] = {0.f, 0.f, (float)(w - 1), 0.f, 0.f, (float)(h - 1), (float)(w - 1), (float)(h - 1)};
    double cc[2][2];
    for (int k = 0; k < 2; k++) {
        const double *Ri = k == 0 ? r1 : r2;
        const UndistortModel m = undistort_model(Ks[k], cs[k].k, 8, nullptr, nullptr);
        double px[4], py[4];
        for (int i = 0; i < 4; i++) {
            double x, y;
            undistort_one(m, (double)corners[2 * i], (double)corners[2 * i + 1], &x, &y);
            x = (double)(float)x;
            y = (double)(float)y;
            const double X = (Ri[0] * x + Ri[1] * y) + Ri[2], Y = (Ri[3] * x + Ri[4] * y) + Ri[5];
            const double W = (Ri[6] * x + Ri[7] * y) + Ri[8];
            px[i] = (double)(float)((X / W) * fc_new + 0.0);
            py[i] = (double)(float)((Y / W) * fc_new + 0.0);
        }
        const double sx = ((px[0] + px[1]) + px[2]) + px[3], sy = ((py[0] + py[1]) + py[2]) + py[3];
        cc[k][0] = (w - 1) / 2.0 - sx * 0.25;
        cc[k][1] = (h - 1) / 2.0 - sy * 0.25;
    }
    // 7.
    if (flags & CALIB_ZERO_DISPARITY) {
        for (int a = 0; a < 2; a++)
            cc[0][a] = cc[1][a] = (cc[0][a] + cc[1][a]) * 0.5;
    } else {
        cc[0][idx ^ 1] = cc[1][idx ^ 1] = (cc[0][idx ^ 1] + cc[1][idx ^ 1]) * 0.5;
    }
    // 8., 9.
    for (int i = 0; i < 9; i++)
        R1[i] = r1[i], R2[i] = r2[i];
    for (int i = 0; i < 12; i++)
        P1[i] = P2[i] = 0.0;
    P1[0] = P1[5] = P2[0] = P2[5] = fc_new;
    P1[2] = cc[0][0], P1[6] = cc[0][1], P2[2] = cc[1][0], P2[6] = cc[1][1];
    P1[10] = P2[10] = 1.0;
    P2[4 * idx + 3] = t[idx] * fc_new;
    for (int i = 0; i < 16; i++)
        Q[i] = 0.0;
    Q[0] = Q[5] = 1.0;
    Q[3] = -cc[0][0], Q[7] = -cc[0][1], Q[11] = fc_new;
    Q[14] = -1.0 / t[idx];
    Q[15] = (cc[0][idx] - cc[1][idx]) / t[idx];
    return nullptr;
}

// 0, 1 (SVO_ERR_ARG) or 2 (SVO_ERR_CAPACITY) with *why set: the sizes of a map and of its source, `images` of them in a call
inline int check_sizes(int w, int h, int src_w, int src_h, int images, const char **why)
{
    *why = nullptr;
    if (w <= 0 || h <= 0 || src_w <= 0 || src_h <= 0)
        return *why = "w, h, src_w and src_h must be positive", 1;
    if (w > MAX_DIM || h > MAX_DIM || src_w > MAX_DIM || src_h > MAX_DIM)
        return *why = "w, h, src_w and src_h may be 32767 at most: the map holds int16 coordinates", 2;
    if ((long long)w * h * images > MAX_PIXELS || (long long)src_w * src_h * images > MAX_PIXELS)
        return *why = "more than 2^30 pixels in one call", 2;
    return 0;
}

// svo_rectify_map_create's model: iR = (P[:, :3] R)^-1 (N9); 0, or the reason
inline const char *map_model(const double *K9, const double *D, int nD, const double *R9, const double *P12, MapModel *out)
{
    if (const char *why = check_camera(K9, D, nD))
        return why;
    if ((R9 && !finite_all(R9, 9)) || (P12 && !finite_all(P12, 12)))
        return "R and P must be finite";
    double Pm[9], PR[9];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++)
            Pm[3 * r + c] = P12 ? P12[4 * r + c] : K9[3 * r + c];
    if (R9)
        mat3(Pm, R9, PR);
    else
        for (int i = 0; i < 9; i++)
            PR[i] = Pm[i];
    if (!inv3(PR, out->iR))
        return "P[:, :3] R is singular";
    out->K4[0] = K9[0], out->K4[1] = K9[4], out->K4[2] = K9[2], out->K4[3] = K9[5];
    out->c = coeffs(D, nD);
    return nullptr;
}

// the device map: rows of `pitch` elements, a multiple of QUAD, so that a thread's four xy words are one aligned 16-byte load
// and its four fraction words one aligned 8-byte load; the pad elements are never read for a pixel that is written
inline int map_pitch(int w) { return (w + QUAD - 1) / QUAD * QUAD; }
inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
inline size_t map_frac_offset(int w, int h) { return align256((size_t)map_pitch(w) * h * 4); }
inline size_t map_bytes(int w, int h) { return map_frac_offset(w, h) + align256((size_t)map_pitch(w) * h * 2); }

struct Grid {
    unsigned x, y, z;
};
inline Grid remap_grid(int w, int h, int images)
{
    const int quads = map_pitch(w) / QUAD;
    return Grid{(unsigned)((quads + BLOCK_X - 1) / BLOCK_X), (unsigned)((h + BLOCK_Y - 1) / BLOCK_Y), (unsigned)images};
}

}  // namespace rectify_plan
