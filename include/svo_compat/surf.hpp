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
    const uint8_t *ptrs[16];
    same_size_ptrs(imgs, n, "surfFeatures", ptrs);
    const Mat &first = *imgs[0];
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
// the points of the surviving pairs, in the order of the left image's key points (ratio_match_points).
// `how`: the pairing (sparse_match_points); its default is the reference's block.
inline void surf_ratio_pairs(svo_ctx *ctx, const Mat &im1, const Mat &im2, double hessian, std::vector<Point2f> &pt1,
                             std::vector<Point2f> &pt2, const SparseMatch &how = SparseMatch())
{
    const Mat *imgs[2] = {&im1, &im2};
    std::vector<KeyPoint> kps[2];
    std::vector<float> desc[2];
    surf_features_batch(ctx, imgs, 2, hessian, kps, desc);
    const std::vector<Point2f> xy1 = keypoint_points(kps[0]), xy2 = keypoint_points(kps[1]);
    sparse_match_points(ctx, how, SVO_MATCH_L2_F32, desc[0].data(), desc[1].data(), 64, (int)xy1.size(), (int)xy2.size(),
                        reinterpret_cast<const float *>(xy1.data()), reinterpret_cast<const float *>(xy2.data()), pt1, pt2);
}

}  // namespace svo_compat
