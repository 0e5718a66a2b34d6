// svo_compat/bundleAdjust.hpp -- the hot-path members of the reference's older class
// `visualOdometry` (src/bundleAdjust.cpp:30-614; the file is not in upstream's build, CMakeLists.txt
// lists it only in a comment) on top of the C ABI, with the reference's names and argument meaning.
#pragma once

#include <cstdio>

#include "surf.hpp"
#include "types.hpp"

namespace svo_compat {

class visualOdometry {
  public:
    int baIterations = 10;  // optimizer.optimize(10), src/bundleAdjust.cpp:606
    // what the last BundleAdjust3d2d did: chi2 before / after, final lambda, iterations, trials
    double lastInfo[5] = {0, 0, 0, 0, 0};
    // ---- the stereo side of the class (src/bundleAdjust.cpp:30-60, 236-317, 384-404) ----
    double baseline = 0.54;
    Mat K;                  // 3x3 CV_64F; stereoTriangulate reads K(0,0), K(1,1), K(0,2), K(1,2), as BundleAdjust3d2d does
    int surfHessian = 500;  // xfeatures2d::SURF::create(500), src/bundleAdjust.cpp:240

    explicit visualOdometry(svo_ctx *ctx = nullptr) : ctx_(ctx ? ctx : shared_context()) {}

    // src/bundleAdjust.cpp:551-613.  points by value as upstream; K 3x3, R 3x3, t 3x1, all CV_64F;
    // (R, t) map world points into the camera (what cv::solvePnP returns after Rodrigues).  Only t is
    // written back (:609-611).  Upstream builds g2o's CameraParameters from K(0,0), K(0,2), K(1,2):
    // K(1,1) is not read.
    void BundleAdjust3d2d(std::vector<Point2f> points_2d, std::vector<Point3f> points_3d, Mat &K, Mat &R, Mat &t)
    {
        if (points_2d.size() != points_3d.size() || points_2d.empty())
            throw std::invalid_argument("BundleAdjust3d2d: one 2-D point per 3-D point, at least one");
        const Mat33d Km = mat33_of(K), Rm = mat33_of(R);
        Vec3d tv = vec3_of(t);
        const double K4[4] = {Km(0, 0), Km(1, 1), Km(0, 2), Km(1, 2)};
        check(svo_ba_3d2d(ctx_, reinterpret_cast<const float *>(points_2d.data()),
                          reinterpret_cast<const float *>(points_3d.data()), (int)points_2d.size(), K4, Rm.m, tv.v,
                          baIterations, nullptr, nullptr, lastInfo, SVO_MEM_HOST));
        for (int i = 0; i < 3; i++)  // eigen2cv(trans, t): t keeps its 3x1 shape
            (t.rows == 3 ? t.at<double>(i, 0) : t.at<double>(0, i)) = tv(i);
    }

    // OURS (upstream's README names it as future work): svo_ba_window behind the class's types.  R / t: one 3x3 / 3x1 CV_64F per
    // pose, world -> camera, written back; fixed: one flag per pose (non-zero = held).  Observations CSR by point: point i owns
    // obs_start[i] .. obs_start[i + 1] - 1, each with its pose index and (u, v, u_right), u_right NaN = mono.  K 3x3 CV_64F (both
    // focal lengths are read); bf = fx * baseline.  baIterations, baWindowHuberMono / Stereo are the parameters; lastWindowInfo
    // receives chi2 before / after, lambda, iterations, trials, observations.  Optional: the refined points (3 doubles each) and
    // the final e^T e of every observation.
    double baWindowHuberMono = 0, baWindowHuberStereo = 0;
    double lastWindowInfo[6] = {0, 0, 0, 0, 0, 0};
    void BundleAdjustWindow(std::vector<Mat> &R, std::vector<Mat> &t, const std::vector<unsigned char> &fixed,
                            const std::vector<Point3f> &points_3d, const std::vector<int> &obs_start, const std::vector<int> &obs_pose,
                            const std::vector<float> &obs_uvr, Mat &K, double bf, std::vector<double> *points_out = nullptr,
                            std::vector<double> *obs_chi2 = nullptr)
    {
        const size_t np = R.size(), n = points_3d.size();
        if (np == 0 || t.size() != np || fixed.size() != np || n == 0 || obs_start.size() != n + 1 ||
            obs_uvr.size() != 3 * obs_pose.size() || obs_start.back() != (int)obs_pose.size())
            throw std::invalid_argument("BundleAdjustWindow: one R, t and flag per pose; obs_start of n + 1 entries ending at the "
                                        "observation count; three floats per observation");
        std::vector<double> poses(12 * np);
        for (size_t j = 0; j < np; j++) {
            const Mat33d Rm = mat33_of(R[j]);
            const Vec3d tv = vec3_of(t[j]);
            for (int k = 0; k < 9; k++)
                poses[12 * j + k] = Rm.m[k];
            for (int k = 0; k < 3; k++)
                poses[12 * j + 9 + k] = tv(k);
        }
        const Mat33d Km = mat33_of(K);
        svo_ba_window_params prm;
        svo_ba_window_default_params(&prm);
        prm.fx = Km(0, 0);
        prm.fy = Km(1, 1);
        prm.cx = Km(0, 2);
        prm.cy = Km(1, 2);
        prm.bf = bf;
        prm.iterations = baIterations;
        prm.huber_mono = baWindowHuberMono;
        prm.huber_stereo = baWindowHuberStereo;
        if (points_out)
            points_out->assign(3 * n, 0.0);
        if (obs_chi2)
            obs_chi2->assign(obs_pose.size(), 0.0);
        check(svo_ba_window(ctx_, &prm, (int)np, poses.data(), fixed.data(), (int)n, reinterpret_cast<const float *>(points_3d.data()),
                            obs_start.data(), obs_pose.data(), obs_uvr.data(), points_out ? points_out->data() : nullptr,
                            obs_chi2 && !obs_chi2->empty() ? obs_chi2->data() : nullptr, lastWindowInfo, SVO_MEM_HOST));
        for (size_t j = 0; j < np; j++) {
            for (int r = 0; r < 3; r++) {
                for (int c = 0; c < 3; c++)
                    R[j].at<double>(r, c) = poses[12 * j + 3 * r + c];
                (t[j].rows == 3 ? t[j].at<double>(r, 0) : t[j].at<double>(0, r)) = poses[12 * j + 9 + r];
            }
        }
    }

    // detector->detect(img, kps) + detector->compute(img, kps, desc) with SURF::create(surfHessian): 64 floats per key point
    void surfFeatures(const Mat &img, std::vector<KeyPoint> &kps, std::vector<float> &desc)
    {
        const Mat *imgs[1] = {&img};
        surf_features_batch(ctx_, imgs, 1, (double)surfHessian, &kps, &desc);
    }

    // src/bundleAdjust.cpp:236-317: SURF on both images, knnMatch(2), ratio 0.8, triangulatePoints with K[I|0] and
    // K[I|(-baseline, 0, 0)], dehomogenised in float.  No F-matrix filter: upstream has none here.  The drawing
    // (drawDeltas, :306-313) is display code and is left out.
    void stereoTriangulate(Mat im1, Mat im2, std::vector<Point3f> &ref3dPts, std::vector<Point2f> &ref2dPts)
    {
        if (mat_data(im1) == nullptr || mat_data(im2) == nullptr) {
            std::printf("NULL IMG\n");  // :242-245
            return;
        }
        const Mat33d Km = mat33_of(K);
        std::vector<Point2f> pt1, pt2;
        surf_ratio_pairs(ctx_, im1, im2, (double)surfHessian, pt1, pt2);
        std::vector<Point3f> pts3d(pt1.size());
        if (!pt1.empty()) {
            double P1[12], P2[12];
            check(svo_stereo_projections(Km(0, 0), Km(1, 1), Km(0, 2), Km(1, 2), baseline, P1, P2));
            check(svo_triangulate(ctx_, P1, P2, reinterpret_cast<const float *>(pt1.data()), reinterpret_cast<const float *>(pt2.data()),
                                  (int)pt1.size(), reinterpret_cast<float *>(pts3d.data()), nullptr, SVO_MEM_HOST));
        }
        ref3dPts = pts3d;
        ref2dPts = pt1;
    }

    // src/bundleAdjust.cpp:384-404: the new pair's points through the 3x4 CV_64F inv_transform.  Upstream writes the three rows
    // out in double and stores floats; svo_transform_points is that arithmetic (the kernel of update3dtransformation), used here.
    // `start` is not read upstream either.
    void relocalizeFrames(int start, Mat imL, Mat imR, Mat &inv_transform, std::vector<Point2f> &ftrPts, std::vector<Point3f> &pts3d)
    {
        (void)start;
        std::vector<Point2f> new2d;
        std::vector<Point3f> new3d;
        ftrPts.clear();
        pts3d.clear();
        stereoTriangulate(imL, imR, new3d, new2d);
        const Mat34d T = mat34_of(inv_transform);
        pts3d.assign(new3d.size(), Point3f());
        if (!new3d.empty())
            check(svo_transform_points(ctx_, T.m, reinterpret_cast<const float *>(new3d.data()), (int)new3d.size(),
                                       reinterpret_cast<float *>(pts3d.data()), SVO_MEM_HOST));
        ftrPts = new2d;
    }

    // src/bundleAdjust.cpp:359, the copy of include/monoUtils.h:195-213: the indices of newref2dFeatures with no listed base point
    // within `radius`.  A negative radius keeps everything upstream (no norm is below it); it is passed on as 0, which does too.
    std::vector<int> removeDuplicates(std::vector<Point2f> &baseref2dFeatures, std::vector<Point2f> &newref2dFeatures,
                                      std::vector<int> &mask, int radius = 10)
    {
        return remove_duplicates(ctx_, baseref2dFeatures, newref2dFeatures, mask, radius < 0 ? 0 : radius);
    }

  private:
    svo_ctx *ctx_;
};

}  // namespace svo_compat
