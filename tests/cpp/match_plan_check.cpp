// The host arithmetic of csrc/match.hip's cross-check, radius and gated searches (match_plan.hip.h) on its own: built with
// -fsanitize=address,undefined and run on the CPU by tests/test_match_ext_abi.py.  Prints "match plan check ok".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../ros_stereo_slam_amd/csrc/match_plan.hip.h"

namespace mp = match_plan;

#define REQUIRE(c)                                                  \
    do {                                                            \
        if (!(c)) {                                                 \
            std::printf("%s:%d failed: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                               \
        }                                                           \
    } while (0)

static float fbits(uint32_t k)
{
    float f;
    memcpy(&f, &k, 4);
    return f;
}

int main()
{
    // rows
    REQUIRE(mp::words(SVO_MATCH_L2_F32, 1) == 1 && mp::words(SVO_MATCH_L2_F32, 256) == 256 && mp::words(SVO_MATCH_L2_F32, 257) == 0);
    REQUIRE(mp::words(SVO_MATCH_L2_U8, 4) == 1 && mp::words(SVO_MATCH_L2_U8, 256) == 64 && mp::words(SVO_MATCH_L2_U8, 6) == 0);
    REQUIRE(mp::words(SVO_MATCH_HAMMING, 16) == 16 && mp::words(SVO_MATCH_HAMMING, 17) == 0 && mp::words(3, 8) == 0 && mp::words(-1, 8) == 0);
    REQUIRE(mp::words(SVO_MATCH_L2_F32, 0) == 0 && mp::words(SVO_MATCH_L2_U8, 0) == 0 && mp::words(SVO_MATCH_HAMMING, 0) == 0);

    // offsets
    int lo = -1, hi = -1;
    bool big = false;
    const int ok[4] = {2, 2, 32770, 32771}, down[3] = {0, 5, 4}, neg[2] = {-1, 3}, over[2] = {0, 32769};
    REQUIRE(mp::check_offsets(nullptr, 1, &lo, &hi, &big) && lo == -1);
    REQUIRE(mp::check_offsets(down, 2, &lo, &hi, &big) && mp::check_offsets(neg, 1, &lo, &hi, &big) && lo == -1 && !big);
    REQUIRE(!mp::check_offsets(ok, 3, &lo, &hi, &big) && lo == 2 && hi == 32771 && !big);
    REQUIRE(!mp::check_offsets(over, 1, &lo, &hi, &big) && big);

    // the split: svo_knn_match's numbers, and every tile of every problem owned by exactly one workgroup
    {
        const int qo[2] = {0, 3}, to[2] = {0, 2049};
        const mp::Search s = mp::plan(qo, to, 1, false);
        REQUIRE(s.qblocks == 1 && s.tiles_max == 65 && s.nsplit == 64 && s.nq_max == 3 && s.nt_max == 2049);
        const mp::Search r = mp::plan(qo, to, 1, true);
        REQUIRE(r.nq[0] == 2049 && r.nt[0] == 3 && r.qblocks == 9 && r.nsplit == 1 && r.q0[0] == 0);
    }
    {
        const int qo[2] = {0, 1000}, to[2] = {0, 1000};
        REQUIRE(mp::plan(qo, to, 1, false).nsplit == 32);  // 4 query blocks -> 256 workgroups per block, 32 tiles
        const int none[2] = {0, 0};
        const mp::Search e = mp::plan(none, to, 1, false);
        REQUIRE(e.qblocks == 0 && e.nsplit == 1);
        REQUIRE(mp::plan(qo, none, 1, false).nsplit == 1);
    }
    for (int nq : {1, 255, 256, 257, 5000, 32768})
        for (int nt : {0, 1, 31, 32, 33, 65, 2049, 32768}) {
            const int qo[3] = {7, 7 + nq, 7 + nq + 5}, to[3] = {0, nt, nt + 40};
            const mp::Search s = mp::plan(qo, to, 2, false);
            REQUIRE(s.nsplit >= 1 && s.nsplit <= mp::MAX_SPLIT && s.q0[0] == 7 && s.nq[1] == 5 && s.nt[1] == 40 && s.q0[15] == 7);
            for (int p = 0; p < 2; p++) {
                const int ntiles = (s.nt[p] + mp::MT - 1) / mp::MT, per = (ntiles + s.nsplit - 1) / s.nsplit;
                std::vector<int> owner(ntiles, 0);
                for (int y = 0; y < s.nsplit; y++)
                    for (int t = y * per; t < (y * per + per < ntiles ? y * per + per : ntiles); t++)
                        owner[t]++;
                for (int t = 0; t < ntiles; t++)
                    REQUIRE(owner[t] == 1);
            }
        }

    // the radius as a key
    REQUIRE(mp::radius_key_max(SVO_MATCH_L2_F32, -1.f) == -1 && mp::radius_key_max(SVO_MATCH_L2_F32, NAN) == -1);
    REQUIRE(mp::radius_key_max(SVO_MATCH_HAMMING, -0.5f) == -1 && mp::radius_key_max(SVO_MATCH_HAMMING, 0.f) == 0);
    REQUIRE(mp::radius_key_max(SVO_MATCH_HAMMING, 2.999f) == 2 && mp::radius_key_max(SVO_MATCH_HAMMING, 3.f) == 3);
    REQUIRE(mp::radius_key_max(SVO_MATCH_HAMMING, INFINITY) == 512 && mp::radius_key_max(SVO_MATCH_HAMMING, 1e30f) == 512);
    REQUIRE(mp::radius_key_max(SVO_MATCH_L2_U8, 0.f) == 0 && mp::radius_key_max(SVO_MATCH_L2_U8, 1.f) == 1);
    REQUIRE(mp::radius_key_max(SVO_MATCH_L2_U8, INFINITY) == (1 << 24) - 1 && mp::radius_key_max(SVO_MATCH_L2_U8, 1e30f) == (1 << 24) - 1);
    REQUIRE(mp::radius_key_max(SVO_MATCH_L2_F32, INFINITY) == 0x7f800000 && mp::radius_key_max(SVO_MATCH_L2_F32, 0.f) == 0);
    REQUIRE(mp::radius_key_max(SVO_MATCH_L2_F32, 3e38f) == 0x7f7fffff);
    // the definition, on both sides of the answer: the key passes, the next one does not
    const float radii[] = {1e-30f, 1e-22f, 1.17549435e-38f, 0.1f, 0.5f, 1.f, 1.4142135f, 3.f, 255.f, 1000.5f, 4079.9f, 4080.f, 65536.f, 1e19f, 1.8446743e19f};
    for (float r : radii) {
        const int64_t kf = mp::radius_key_max(SVO_MATCH_L2_F32, r);
        REQUIRE(kf >= 0 && kf < 0x7f800000 && mp::dist_of_key(SVO_MATCH_L2_F32, (uint32_t)kf) <= r);
        REQUIRE(mp::dist_of_key(SVO_MATCH_L2_F32, (uint32_t)kf + 1) > r);
        const int64_t ku = mp::radius_key_max(SVO_MATCH_L2_U8, r);
        REQUIRE(ku >= 0 && mp::dist_of_key(SVO_MATCH_L2_U8, (uint32_t)ku) <= r);
        REQUIRE(ku == (1 << 24) - 1 || mp::dist_of_key(SVO_MATCH_L2_U8, (uint32_t)ku + 1) > r);
    }
    // every radius that is the root of an integer key near the top, where neighbouring keys share a rooted float
    int shared = 0;
    for (uint32_t k = 16646400 - 3000; k <= 16646400; k++) {
        const float r = mp::dist_of_key(SVO_MATCH_L2_U8, k);
        const int64_t m = mp::radius_key_max(SVO_MATCH_L2_U8, r);
        REQUIRE(m >= (int64_t)k && mp::dist_of_key(SVO_MATCH_L2_U8, (uint32_t)m) == r && mp::dist_of_key(SVO_MATCH_L2_U8, (uint32_t)m + 1) > r);
        shared += m > (int64_t)k;
        const int64_t below = mp::radius_key_max(SVO_MATCH_L2_U8, nextafterf(r, 0.f));
        REQUIRE(below < (int64_t)k && mp::dist_of_key(SVO_MATCH_L2_U8, (uint32_t)below + 1) >= r);
    }
    REQUIRE(shared > 100);
    for (uint32_t k = 0x3f800000u - 40; k < 0x3f800000u + 40; k++) {   // float keys around 1
        const float r = mp::dist_of_key(SVO_MATCH_L2_F32, k);
        const int64_t m = mp::radius_key_max(SVO_MATCH_L2_F32, r);
        REQUIRE(m >= (int64_t)k && mp::dist_of_key(SVO_MATCH_L2_F32, (uint32_t)m) == r && fbits((uint32_t)m + 1) > fbits((uint32_t)m));
    }

    // mask offsets, the CSR verdict, the sort
    {
        const int qo[4] = {3, 3, 32771, 32772}, to[4] = {0, 9, 32777, 32777};
        uint64_t off[4];
        mp::mask_offsets(qo, to, 3, off);
        REQUIRE(off[0] == 0 && off[1] == 0 && off[2] == (uint64_t)32768 * 32768 && off[3] == off[2]);
        std::vector<int> q16(17), t16(17);
        for (int p = 0; p <= 16; p++)
            q16[p] = t16[p] = p * 32768;
        uint64_t o16[17];
        mp::mask_offsets(q16.data(), t16.data(), 16, o16);
        REQUIRE(o16[16] == (uint64_t)16 << 30);   // beyond 32 bits
    }
    REQUIRE(mp::saturate(0) == 0 && mp::saturate(INT_MAX) == INT_MAX && mp::saturate((uint64_t)INT_MAX + 1) == INT_MAX);
    REQUIRE(mp::saturate((uint64_t)16 << 30) == INT_MAX);
    REQUIRE(mp::csr_fits(0, 0, 0) == 1 && mp::csr_fits(10, 10, 10) == 1 && mp::csr_fits(11, 10, 10) == 0);
    REQUIRE(mp::csr_fits(8192, 8192, 8192) == 1 && mp::csr_fits(8193, 8193, 1 << 20) == 0 && mp::csr_fits((uint64_t)1 << 34, 1, INT_MAX) == 0);
    REQUIRE(mp::csr_fits(0, 0, -1) == 0);
    REQUIRE(mp::sort_width(1) == 1 && mp::sort_width(2) == 2 && mp::sort_width(3) == 4 && mp::sort_width(4097) == 8192 && mp::sort_width(8192) == 8192);
    REQUIRE(mp::sort_lds(0) == 8 && mp::sort_lds(1000) == 8192 && mp::sort_lds(32768) == 65536 && mp::sort_lds(8193) == 65536);
    std::printf("match plan check ok\n");
    return 0;
}
