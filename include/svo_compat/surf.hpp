// svo_compat/surf.hpp -- xfeatures2d::SURF::create(hessian) -> detect / compute and the pairing that follows it in both of the
// reference's SURF users (src/bundleAdjust.cpp:240-280, include/trangulation.h:33-61), on top of svo_surf_extract_batch,
// svo_knn_match and svo_ratio_pairs.  Shared by visualOdometry (bundleAdjust.hpp) and visualSLAM (visualSLAM.hpp).
#pragma once

#include "types.hpp"

namespace svo_compat {

// n (1 ... 16) images of one size through one svo_surf_extract_batch call; desc == nullptr: detect only.  The capacity grows to
// what the library asks for, so a call never loses key points.
inline void surf_features_batch(svo_ctx *ctx, const Mat *const *imgs, int n, double hessian, std::vector<KeyPoint> *kps,
                                std::vector<float> *desc)
{
    const Mat &first = *imgs[0];
    const uint8_t *ptrs[16];
    if (n < 1 || n > 16)
        throw SvoError(SVO_ERR_ARG, "surfFeatures: 1 ... 16 images per call");
    for (int i = 0; i < n; i++) {
        if (mat_cols(*imgs[i]) != mat_cols(first) || mat_rows(*imgs[i]) != mat_rows(first) ||
            mat_channels(*imgs[i]) != mat_channels(first))
            throw SvoError(SVO_ERR_ARG, "surfFeatures: the images differ in size");
        ptrs[i] = mat_data(*imgs[i]);
    }
    svo_surf_params prm;
    svo_surf_default_params(&prm);
    prm.hessian_threshold = hessian;
    size_t cap = 8192;
    std::vector<float> xy, size, angle, resp, d;
    std::vector<int> oct, lap, cnt((size_t)n);
    for (int attempt = 0;; attempt++) {
        const size_t e = cap * (size_t)n;
        xy.assign(2 * e, 0.f);
        size.assign(e, 0.f);
        angle.assign(e, 0.f);
        resp.assign(e, 0.f);
        d.assign(desc ? 64 * e : 0, 0.f);
        oct.assign(e, 0);
        lap.assign(e, 0);
        const int rc = svo_surf_extract_batch(ctx, ptrs, n, mat_cols(first), mat_rows(first), mat_channels(first), &prm, (int)cap,
                                              xy.data(), size.data(), angle.data(), resp.data(), oct.data(), lap.data(),
                                              desc ? d.data() : nullptr, cnt.data(), SVO_MEM_HOST);
        size_t need = 0;
        for (int i = 0; i < n; i++)
            need = (size_t)cnt[(size_t)i] > need ? (size_t)cnt[(size_t)i] : need;
        if (rc == SVO_ERR_CAPACITY && attempt == 0 && need > cap && need <= 65536) {
            cap = need;   // case (a) of svo.h: every count is the needed one
            continue;
        }
        check(rc);
        break;
    }
    for (int i = 0; i < n; i++) {
        const size_t b = cap * (size_t)i, m = (size_t)cnt[(size_t)i];
        kps[i].assign(m, KeyPoint());
        for (size_t j = 0; j < m; j++) {
            KeyPoint &k = kps[i][j];
            k.pt = Point2f(xy[2 * (b + j)], xy[2 * (b + j) + 1]);
            k.size = size[b + j];
            k.angle = angle[b + j];
            k.response = resp[b + j];
            k.octave = oct[b + j];
            k.class_id = lap[b + j];
        }
        if (desc)
            desc[i].assign(d.begin() + 64 * b, d.begin() + 64 * (b + m));
    }
}

// SURF on both images (one set of launches), BFMatcher().knnMatch(desc1, desc2, matches, 2), m.distance < 0.8 * n.distance:
// the points of the surviving pairs, in the order of the left image's key points.  Fewer than two key points on the right give no
// pair (upstream would read matches[i][1] of a one-element list).
inline void surf_ratio_pairs(svo_ctx *ctx, const Mat &im1, const Mat &im2, double hessian, std::vector<Point2f> &pt1,
                             std::vector<Point2f> &pt2)
{
    const Mat *imgs[2] = {&im1, &im2};
    std::vector<KeyPoint> kps[2];
    std::vector<float> desc[2];
    surf_features_batch(ctx, imgs, 2, hessian, kps, desc);
    pt1.clear();
    pt2.clear();
    const int n1 = (int)kps[0].size(), n2 = (int)kps[1].size();
    if (n1 < 1 || n2 < 2)
        return;
    std::vector<float> a(2 * (size_t)n1), b(2 * (size_t)n2);
    for (int i = 0; i < n1; i++) {
        a[2 * (size_t)i] = kps[0][(size_t)i].pt.x;
        a[2 * (size_t)i + 1] = kps[0][(size_t)i].pt.y;
    }
    for (int i = 0; i < n2; i++) {
        b[2 * (size_t)i] = kps[1][(size_t)i].pt.x;
        b[2 * (size_t)i + 1] = kps[1][(size_t)i].pt.y;
    }
    const int qo[2] = {0, n1}, to[2] = {0, n2};
    std::vector<int> idx((size_t)n1 * 2);
    std::vector<float> dist((size_t)n1 * 2);
    check(svo_knn_match(ctx, SVO_MATCH_L2_F32, desc[0].data(), desc[1].data(), 64, qo, to, 1, 2, idx.data(), dist.data(),
                        SVO_MEM_HOST));
    pt1.assign((size_t)n1, Point2f());
    pt2.assign((size_t)n1, Point2f());
    int cnt = 0;
    check(svo_ratio_pairs(ctx, idx.data(), dist.data(), n1, 2, 0.8, a.data(), b.data(), reinterpret_cast<float *>(pt1.data()),
                          reinterpret_cast<float *>(pt2.data()), nullptr, &cnt, SVO_MEM_HOST));
    pt1.resize((size_t)cnt);
    pt2.resize((size_t)cnt);
}

}  // namespace svo_compat
