// ba_window_plan_check.cpp -- the host arithmetic of csrc/ba_window.hip (ba_window_plan.hip.h: the refusals and the CSR validation, the
// numbering of the free poses, the slab geometry, the packed triangle index, the LM rule) exercised on its own;
// tests/test_ba_window_abi.py builds it with -fsanitize=address,undefined and runs it.  No GPU.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../ros_stereo_slam_amd/csrc/ba_window_plan.hip.h"

using namespace ba_window_plan;

#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            return 1;                                                         \
        }                                                                     \
    } while (0)

static bool says(const char *why, const char *word) { return why && std::strstr(why, word); }

int main()
{
    svo_ba_window_params prm = {700, 700, 300, 200, 350, 10, 0, 0};
    int token = 0;
    const void *p = &token;
    Plan pl;
    std::vector<uint8_t> fixed(40, 0);
    // ---- scalars, the numbering of the free poses ----
    fixed[0] = 1;
    EXPECT(!check_scalars(&prm, 3, p, fixed.data(), 5, p, p, p, p, SVO_MEM_HOST, &pl));
    EXPECT(pl.n_free == 2 && pl.free_index[0] == -1 && pl.free_index[1] == 0 && pl.free_index[2] == 1 && pl.free_list[0] == 1 &&
           pl.free_list[1] == 2);
    EXPECT(says(check_scalars(nullptr, 3, p, fixed.data(), 5, p, p, p, p, SVO_MEM_HOST, &pl), "null"));
    EXPECT(says(check_scalars(&prm, 3, nullptr, fixed.data(), 5, p, p, p, p, SVO_MEM_HOST, &pl), "null"));
    EXPECT(says(check_scalars(&prm, 3, p, nullptr, 5, p, p, p, p, SVO_MEM_HOST, &pl), "null"));
    EXPECT(says(check_scalars(&prm, 3, p, fixed.data(), 5, nullptr, p, p, p, SVO_MEM_HOST, &pl), "null"));
    EXPECT(says(check_scalars(&prm, 3, p, fixed.data(), 5, p, nullptr, p, p, SVO_MEM_HOST, &pl), "null"));
    EXPECT(says(check_scalars(&prm, 3, p, fixed.data(), 5, p, p, nullptr, p, SVO_MEM_HOST, &pl), "null"));
    EXPECT(says(check_scalars(&prm, 3, p, fixed.data(), 5, p, p, p, nullptr, SVO_MEM_HOST, &pl), "null"));
    for (int mem : {-1, 2})
        EXPECT(says(check_scalars(&prm, 3, p, fixed.data(), 5, p, p, p, p, mem, &pl), "mem"));
    for (int np : {0, -1, 33})
        EXPECT(says(check_scalars(&prm, np, p, fixed.data(), 5, p, p, p, p, SVO_MEM_HOST, &pl), "n_poses"));
    for (int n : {0, -7})
        EXPECT(says(check_scalars(&prm, 3, p, fixed.data(), n, p, p, p, p, SVO_MEM_HOST, &pl), "n_points"));
    EXPECT(says(check_scalars(&prm, 3, p, fixed.data(), MAX_POINTS + 1, p, p, p, p, SVO_MEM_HOST, &pl), "at most 2^20"));
    EXPECT(!check_scalars(&prm, 3, p, fixed.data(), MAX_POINTS, p, p, p, p, SVO_MEM_HOST, &pl));
    prm.iterations = -1;
    EXPECT(says(check_scalars(&prm, 3, p, fixed.data(), 5, p, p, p, p, SVO_MEM_HOST, &pl), "iterations"));
    prm.iterations = 0;
    EXPECT(!check_scalars(&prm, 3, p, fixed.data(), 5, p, p, p, p, SVO_MEM_HOST, &pl));
    prm.huber_mono = -1;
    EXPECT(says(check_scalars(&prm, 3, p, fixed.data(), 5, p, p, p, p, SVO_MEM_HOST, &pl), "Huber"));
    prm.huber_mono = 0;
    prm.huber_stereo = std::nan("");
    EXPECT(says(check_scalars(&prm, 3, p, fixed.data(), 5, p, p, p, p, SVO_MEM_HOST, &pl), "Huber"));
    prm.huber_stereo = 0;
    EXPECT(says(check_scalars(&prm, 18, p, fixed.data(), 5, p, p, p, p, SVO_MEM_HOST, &pl), "more than 16"));   // 17 free
    EXPECT(!check_scalars(&prm, 17, p, fixed.data(), 5, p, p, p, p, SVO_MEM_HOST, &pl) && pl.n_free == 16);
    for (int j = 16; j < 32; j++)
        fixed[j] = 1;
    fixed[0] = 0;
    EXPECT(!check_scalars(&prm, 32, p, fixed.data(), 5, p, p, p, p, SVO_MEM_HOST, &pl) && pl.n_free == 16 && pl.free_list[15] == 15 &&
           pl.free_index[31] == -1);
    std::vector<uint8_t> held(32, 7);
    EXPECT(says(check_scalars(&prm, 32, p, held.data(), 5, p, p, p, p, SVO_MEM_HOST, &pl), "no free pose"));

    // ---- the CSR arrays: two poses, pose 0 held ----
    const uint8_t fx2[2] = {1, 0};
    const float nanf_ = std::nanf("");
    {
        const int start[5] = {0, 2, 3, 3, 5}, pose[5] = {0, 1, 1, 0, 1};
        float uvr[15];
        for (int o = 0; o < 5; o++) {
            uvr[3 * o] = 10.f * o;
            uvr[3 * o + 1] = 5.f;
            uvr[3 * o + 2] = pose[o] == 0 ? 3.f : nanf_;
        }
        EXPECT(!check_scalars(&prm, 2, p, fx2, 4, p, start, pose, uvr, SVO_MEM_HOST, &pl));
        EXPECT(!check_starts(4, start));
        EXPECT(!check_csr(&prm, 2, 4, start, pose, uvr, &pl));
        EXPECT(pl.n_obs == 5 && pl.n_stereo == 2 && pl.pose_obs[0] == 2 && pl.pose_obs[1] == 3);
        prm.bf = 0;
        EXPECT(says(check_csr(&prm, 2, 4, start, pose, uvr, &pl), "bf"));
        prm.bf = std::nan("");
        EXPECT(says(check_csr(&prm, 2, 4, start, pose, uvr, &pl), "bf"));
        for (int o = 0; o < 5; o++)
            uvr[3 * o + 2] = nanf_;
        EXPECT(!check_csr(&prm, 2, 4, start, pose, uvr, &pl) && pl.n_stereo == 0);   // mono only: bf is not read
        prm.bf = 350;
        const int twice[5] = {0, 0, 1, 0, 1}, far[5] = {0, 1, 2, 0, 1}, neg[5] = {0, 1, -1, 0, 1};
        EXPECT(says(check_csr(&prm, 2, 4, start, twice, uvr, &pl), "twice"));
        EXPECT(says(check_csr(&prm, 2, 4, start, far, uvr, &pl), "out of range"));
        EXPECT(says(check_csr(&prm, 2, 4, start, neg, uvr, &pl), "out of range"));
        const int few[5] = {0, 1, 0, 0, 1}, start_few[5] = {0, 2, 3, 3, 5};
        EXPECT(says(check_csr(&prm, 2, 4, start_few, few, uvr, &pl), "fewer than three"));
        const int down[5] = {0, 2, 1, 3, 5}, off[5] = {1, 2, 3, 3, 5}, negs[5] = {0, -1, 3, 3, 5};
        EXPECT(says(check_starts(4, down), "decrease"));
        EXPECT(says(check_starts(4, off), "begin at 0"));
        EXPECT(says(check_starts(4, negs), "decrease"));
        const int big[3] = {0, 1, MAX_OBS + 1};
        EXPECT(says(check_starts(2, big), "at most 2^28"));
    }
    // a pose index of 31 sets the top bit of the mask
    {
        std::vector<uint8_t> f32(32, 1);
        f32[31] = 0;
        std::vector<int> start = {0, 32, 64, 96}, pose;
        std::vector<float> uvr;
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 32; j++) {
                pose.push_back(31 - j);
                uvr.insert(uvr.end(), {1.f, 2.f, nanf_});
            }
        EXPECT(!check_scalars(&prm, 32, p, f32.data(), 3, p, start.data(), pose.data(), uvr.data(), SVO_MEM_HOST, &pl));
        EXPECT(!check_starts(3, start.data()) && !check_csr(&prm, 32, 3, start.data(), pose.data(), uvr.data(), &pl));
        EXPECT(pl.pose_obs[31] == 3 && pl.n_obs == 96);
    }

    // ---- the packed triangle and the slab layout ----
    for (int nf = 1; nf <= MAX_FREE; nf++) {
        const SlabLayout l = slab_layout(nf);
        EXPECT(l.dim == 6 * nf && l.off_sb == tri_size(l.dim) && l.off_hpp == l.off_sb + l.dim && l.off_bp == l.off_hpp + 21 * nf);
        EXPECT(l.off_chi == l.off_bp + l.dim && l.off_max == l.off_chi + 1 && l.stride > l.off_max && l.stride % 8 == 0);
        std::vector<char> hit(tri_size(l.dim), 0);
        for (int r = 0; r < l.dim; r++)
            for (int c = r; c < l.dim; c++) {
                const int k = tri_index(l.dim, r, c);
                EXPECT(k >= 0 && k < tri_size(l.dim) && !hit[k]);
                hit[k] = 1;
            }
        EXPECT(tri_index(l.dim, 0, 0) == 0 && tri_index(l.dim, l.dim - 1, l.dim - 1) == tri_size(l.dim) - 1);
    }
    // the linearise + Schur workgroup's LDS (slab, 32 x (10 + 36) doubles, 64 ints) fits the 64 KB of a workgroup
    EXPECT((slab_layout(MAX_FREE).stride + MAX_POSES * 46) * 8 + 2 * MAX_POSES * 4 <= 65536);
    EXPECT(tri_size(MAX_DIM) == 4656);
    for (int n : {1, CHUNK - 1, CHUNK, CHUNK + 1, BLOCK - 1, BLOCK, BLOCK + 1, 4096, MAX_POINTS}) {
        const long long a = schur_slabs(n), b = backsub_slabs(n);
        EXPECT(a * CHUNK >= n && (a - 1) * CHUNK < n && b * BLOCK >= n && (b - 1) * BLOCK < n);
        EXPECT(a * slab_layout(MAX_FREE).stride * 8 < (1LL << 31) && 3LL * n < (1LL << 31));
    }

    // ---- the LM rule ----
    {
        LmState s;
        s.chi = 100;
        s.lambda = lambda_init(2e5);
        EXPECT(s.lambda == 2.0);
        EXPECT(lm_trial(s, 40, 60, true));   // rho = 60 / 60.001: q ~ 1, alpha ~ 0 -> the factor is 1/3
        EXPECT(s.chi == 40 && s.ni == 2 && std::fabs(s.lambda - 2.0 / 3.0) < 1e-12 && s.qmax == 1 && s.rho > 0.99);
        EXPECT(!lm_trial(s, 50, 60, true));  // chi2 rose
        EXPECT(s.chi == 40 && s.ni == 4 && std::fabs(s.lambda - 4.0 / 3.0) < 1e-12 && s.rho < 0);
        EXPECT(!lm_trial(s, 10, 60, false)); // a failed factorisation is a rejected trial whatever chi2 says
        EXPECT(s.ni == 8 && s.rho < 0 && s.chi == 40);
        EXPECT(!lm_trial(s, std::nan(""), 60, true));
        EXPECT(!lm_trial(s, HUGE_VAL, 60, true));
        EXPECT(s.chi == 40 && s.qmax == 5);
        LmState h;
        h.chi = 100;
        h.lambda = 3;
        EXPECT(lm_trial(h, 99.97, 60, true));   // rho = 0.03 / 60.001: q ~ -1, alpha ~ 2 -> capped at 2/3
        EXPECT(std::fabs(h.lambda - 2.0) < 1e-12);
    }
    std::puts("ba window plan check ok");
    return 0;
}
