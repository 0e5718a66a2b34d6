// The host decisions of csrc/rectify.hip (rectify_plan.hip.h) on their own, for a build with -fsanitize=address,undefined: the
// refusals with untouched outputs, the rectification of a rotated rig (orthonormal rotations, a baseline along one axis), the
// fixed-point conversion at its boundaries (NaN, infinities, 2^31), the undistortion against the forward model, the map layout and
// the launch geometry up to the largest accepted sizes.  Prints "rectify plan check ok".
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../ros_stereo_slam_amd/csrc/rectify_plan.hip.h"

namespace rp = rectify_plan;

#define REQUIRE(cond)                                                      \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                      \
        }                                                                  \
    } while (0)

int main()
{
    const double K1[9] = {458.654, 0, 367.215, 0, 457.296, 248.375, 0, 0, 1}, K2[9] = {457.587, 0, 379.999, 0, 456.134, 255.238, 0, 0, 1};
    const double D1[4] = {-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05}, D2[4] = {-0.28368365, 0.07451284, -0.00010473, -3.555907e-05};
    double R[9];
    const double om[3] = {0.003, -0.017, 0.002}, T[3] = {-0.110, 0.0004, -0.0009};
    rp::rodrigues_matrix(om, R);
    double back[3];
    rp::rodrigues_vector(R, back);
    for (int i = 0; i < 3; i++)
        REQUIRE(std::fabs(back[i] - om[i]) < 1e-12);

    double R1[9], R2[9], P1[12], P2[12], Q[16];
    REQUIRE(rp::stereo_rectify(K1, D1, 4, K2, D2, 4, 752, 480, R, T, rp::CALIB_ZERO_DISPARITY, -1.0, 0, 0, R1, R2, P1, P2, Q) == nullptr);
    for (const double *M : {R1, R2})
        for (int a = 0; a < 3; a++)
            for (int b = 0; b < 3; b++) {
                double s = 0;
                for (int k = 0; k < 3; k++)
                    s += M[3 * a + k] * M[3 * b + k];
                REQUIRE(std::fabs(s - (a == b)) < 1e-14);
            }
    double t[3];
    rp::mat3v(R2, T, t);
    REQUIRE(std::fabs(t[1]) < 1e-12 && std::fabs(t[2]) < 1e-12 && t[0] < 0 && P2[3] == t[0] * P1[0] && P2[7] == 0 && Q[15] == 0);
    const double Tv[3] = {0.001, -0.2, 0.0};
    REQUIRE(rp::stereo_rectify(K1, D1, 4, K2, nullptr, 0, 752, 480, R, Tv, 0, -1.0, 376, 240, R1, R2, P1, P2, Q) == nullptr);
    REQUIRE(P2[7] != 0 && P2[3] == 0 && P1[2] == P2[2]);  // a vertical rig: idx = 1, x shared without ZERO_DISPARITY

    // refusals: nothing written
    double o[5][16];
    auto fresh = [&] { for (auto &m : o) for (double &v : m) v = 7.0; };
    auto untouched = [&] { for (auto &m : o) for (double v : m) if (v != 7.0) return false; return true; };
    const double nan = std::numeric_limits<double>::quiet_NaN(), zero3[3] = {0, 0, 0}, Kbad[9] = {nan, 0, 0, 0, 1, 0, 0, 0, 1};
    fresh();
#define REFUSED(...) REQUIRE(rp::stereo_rectify(__VA_ARGS__, o[0], o[1], o[2], o[3], o[4]) != nullptr && untouched())
    REFUSED(nullptr, D1, 4, K2, D2, 4, 752, 480, R, T, 0, -1.0, 0, 0);
    REFUSED(K1, D1, 3, K2, D2, 4, 752, 480, R, T, 0, -1.0, 0, 0);
    REFUSED(K1, D1, 12, K2, D2, 4, 752, 480, R, T, 0, -1.0, 0, 0);
    REFUSED(K1, D1, 4, K2, D2, 14, 752, 480, R, T, 0, -1.0, 0, 0);
    REFUSED(K1, nullptr, 4, K2, D2, 4, 752, 480, R, T, 0, -1.0, 0, 0);
    REFUSED(K1, D1, 4, K2, D2, 4, 0, 480, R, T, 0, -1.0, 0, 0);
    REFUSED(K1, D1, 4, K2, D2, 4, 752, -1, R, T, 0, -1.0, 0, 0);
    REFUSED(K1, D1, 4, K2, D2, 4, 752, 480, R, T, 0, 0.0, 0, 0);
    REFUSED(K1, D1, 4, K2, D2, 4, 752, 480, R, T, 0, 1.0, 0, 0);
    REFUSED(K1, D1, 4, K2, D2, 4, 752, 480, R, T, 0, nan, 0, 0);
    REFUSED(K1, D1, 4, K2, D2, 4, 752, 480, R, T, 0, -1.0, 10, 0);
    REFUSED(K1, D1, 4, K2, D2, 4, 752, 480, R, zero3, 0, -1.0, 0, 0);
    REFUSED(K1, D1, 4, K2, D2, 4, 752, 480, nullptr, T, 0, -1.0, 0, 0);
    REFUSED(Kbad, D1, 4, K2, D2, 4, 752, 480, R, T, 0, -1.0, 0, 0);
    REQUIRE(rp::stereo_rectify(K1, D1, 4, K2, D2, 4, 752, 480, R, T, 0, -1.0, 0, 0, nullptr, o[1], o[2], o[3], o[4]) != nullptr && untouched());

    // the fixed-point conversion
    const double inf = std::numeric_limits<double>::infinity();
    REQUIRE(rp::fix5(1 / 64.) == 0 && rp::fix5(3 / 64.) == 2 && rp::fix5(-1 / 64.) == 0 && rp::fix5(-3 / 64.) == -2);
    REQUIRE(rp::fix5(nan) == INT_MIN && rp::fix5(inf) == INT_MIN && rp::fix5(-inf) == INT_MIN && rp::fix5(1e300) == INT_MIN);
    REQUIRE(rp::fix5(67108864.0) == INT_MIN && rp::fix5(67108863.99) == INT_MIN && rp::fix5(67108863.9) == 2147483645);
    REQUIRE(rp::fix5(-67108864.0) == INT_MIN && rp::fix5(-67108865.0) == INT_MIN);
    short x, y;
    unsigned short f;
    rp::map_words(-1 / 32., 40000.0, &x, &y, &f);
    REQUIRE(x == -1 && y == 32767 && f == 31);
    rp::map_words(nan, -7.25, &x, &y, &f);
    REQUIRE(x == -32768 && y == -8 && f == 24 * 32);

    // the undistortion inverts the model where the distortion is mild, and the host entry refuses as documented
    const double Dm[5] = {-0.05, 0.01, 0.0002, -0.0001, 0.001};
    const rp::UndistortModel um = rp::undistort_model(K1, Dm, 5, nullptr, nullptr);
    const rp::Coeffs cm = rp::coeffs(Dm, 5);
    const double K4[4] = {K1[0], K1[4], K1[2], K1[5]};
    for (double u = 0; u < 752; u += 93.5)
        for (double v = 0; v < 480; v += 79.25) {
            double nx, ny, bu, bv;
            rp::undistort_one(um, u, v, &nx, &ny);
            rp::distort(nx, ny, K4, cm, &bu, &bv);
            REQUIRE(std::fabs(bu - u) < 1e-3 && std::fabs(bv - v) < 1e-3);
        }
    std::vector<float> pts = {10.f, 20.f, 700.f, 400.f};
    std::vector<double> out(4, 7.0);
    REQUIRE(rp::undistort_points_host(pts.data(), 2, K1, D1, 4, R1, P1, out.data()) == nullptr && out[0] != 7.0);
    out.assign(4, 7.0);
    REQUIRE(rp::undistort_points_host(pts.data(), -1, K1, D1, 4, nullptr, nullptr, out.data()) != nullptr);
    REQUIRE(rp::undistort_points_host(pts.data(), 2, K1, D1, 6, nullptr, nullptr, out.data()) != nullptr);
    REQUIRE(rp::undistort_points_host(nullptr, 2, K1, D1, 4, nullptr, nullptr, out.data()) != nullptr);
    REQUIRE(rp::undistort_points_host(pts.data(), 2, Kbad, D1, 4, nullptr, nullptr, out.data()) != nullptr);
    REQUIRE(out[0] == 7.0 && out[3] == 7.0);
    REQUIRE(rp::undistort_points_host(nullptr, 0, K1, nullptr, 0, nullptr, nullptr, nullptr) == nullptr);

    // the map model: a singular P R is refused; R = NULL and P = NULL give K's inverse
    rp::MapModel mm;
    const double Rz[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    REQUIRE(rp::map_model(K1, D1, 4, Rz, nullptr, &mm) != nullptr && rp::map_model(K1, D1, 6, nullptr, nullptr, &mm) != nullptr);
    REQUIRE(rp::map_model(K1, D1, 4, nullptr, nullptr, &mm) == nullptr && std::fabs(mm.iR[0] * K1[0] - 1) < 1e-15 && mm.iR[8] == 1.0);
    double u, v;
    rp::map_pixel(mm, 367, 248, &u, &v);
    REQUIRE(std::fabs(u - 367) < 0.01 && std::fabs(v - 248) < 0.01);  // next to the principal point the distortion vanishes

    // sizes, layout and geometry
    const char *why = nullptr;
    REQUIRE(rp::check_sizes(752, 480, 752, 480, 32, &why) == 0 && rp::check_sizes(0, 1, 1, 1, 1, &why) == 1 && why);
    REQUIRE(rp::check_sizes(32768, 1, 1, 1, 1, &why) == 2 && rp::check_sizes(1, 1, 1, 32768, 1, &why) == 2);
    REQUIRE(rp::check_sizes(32767, 32767, 1, 1, 1, &why) == 0 && rp::check_sizes(32767, 32767, 1, 1, 2, &why) == 2);
    REQUIRE(rp::check_sizes(32768, 32768, 1, 1, 1, &why) == 2 && rp::check_sizes(1, 1, 32767, 32767, 2, &why) == 2);
    for (int w : {1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 752, 1241, 32767})
        for (int h : {1, 2, 3, 480, 32767}) {
            const int pitch = rp::map_pitch(w);
            REQUIRE(pitch >= w && pitch < w + rp::QUAD && pitch % rp::QUAD == 0);
            REQUIRE(rp::map_frac_offset(w, h) % 256 == 0 && rp::map_frac_offset(w, h) >= (size_t)pitch * h * 4);
            REQUIRE(rp::map_bytes(w, h) >= rp::map_frac_offset(w, h) + (size_t)pitch * h * 2);
            for (int images : {1, 16, 32}) {
                const rp::Grid g = rp::remap_grid(w, h, images);
                REQUIRE((long long)g.x * rp::BLOCK_X * rp::QUAD >= w && (long long)(g.x - 1) * rp::BLOCK_X * rp::QUAD < w);
                REQUIRE((long long)g.y * rp::BLOCK_Y >= h && g.y <= 65535 && g.z == (unsigned)images && g.z <= 65535);
            }
        }
    std::printf("rectify plan check ok\n");
    return 0;
}
