// svo_compat/stereoCV.hpp -- the reference's StereoProcess (include/stereoCV.h:32-73): stereoTriangulate(im1, im2,
// out3d) on the hot path's sparse stereo, and the dense SGBM demo of src/StereoCV.cpp -- stereoMatch(iter) and
// reprojectDisparity(disp, pts, colours) -- on svo_sgbm_compute / svo_stereo_reproject -- and pclPublish(pts, colours)
// on svo_sor_filter_large, the filtered cloud left in publishedCloud / publishedColors instead of a ROS message --
// and monocularTriangulate(im1, im2, out3d) on svo_find_essential / svo_recover_pose / svo_triangulate; with BRIEF_FLAG
// stereoTriangulate runs the reference's own SIFT + BRIEF sequence (svo_sift_extract_batch / svo_brief_describe_batch).  getImg is
// public here, a thin wrapper over the frame loader.  visualizeCloud and mainLoop are not provided.
#pragma once

#include <cstdint>
#include <cstdio>
#include <memory>
#include <stdexcept>

#include "visualSLAM.hpp"

namespace svo_compat {

class StereoProcess {
  public:
    double baseline = 0.5707;  // include/stereoCV.h:40
    double focal_x = 7.188560000000e+02, cx = 6.071928000000e+02;
    double focal_y = 7.188560000000e+02, cy = 1.852157000000e+02;
    std::vector<Point3f> tri3dPoints, color3dMap;

    explicit StereoProcess(svo_ctx *ctx = nullptr) : slam_(ctx) {}
    // include/stereoCV.h:52-57 (the ROS publisher is not created)
    StereoProcess(const char *lptr, const char *rptr, svo_ctx *ctx = nullptr) : lFptr(lptr), rFptr(rptr), slam_(ctx)
    {
        ctx_ = ctx ? ctx : shared_context();
    }

    // include/stereoCV.h:36-48
    const char *lFptr = nullptr, *rFptr = nullptr;
    Mat lImg, rImg;
    Mat K = k_matrix(focal_x, focal_y, cx, cy);
    // false (default): reprojectDisparity does what the reference does -- Q of stereoRectify with t = +baseline and the
    // raw x16 disparities, which puts every valid pixel behind the camera so that its (0.01, 5] window keeps nothing
    // (DESIGN.md section 10).  true: the conventional Q (t = -baseline) and disparities / 16, metric points.
    bool metricDisparity = false;

    // src/StereoCV.cpp:21-59: both frames loaded as visualSLAM::loadImageL / R do (B,G,R, svo_io_load_frame), converted
    // to grey and matched with StereoSGBM(1, 96, 7, 24, 96, 0, 60, 0, 3000, 5).  Returns CV_16SC1, disparity x 16; an
    // empty Mat when a frame is missing (the reference prints and carries on).
    Mat stereoMatch(int iter)
    {
        lImg = load_bgr(lFptr, iter);
        rImg = load_bgr(rFptr, iter);
        if (lImg.empty() || rImg.empty() || lImg.rows != rImg.rows || lImg.cols != rImg.cols)
            return Mat();
        if (RECTIFY_FLAG) {
            Mat l, r;
            rectifyPair(lImg, rImg, l, r, false);
            lImg = l;
            rImg = r;
        }
        svo_sgbm_params prm;
        svo_sgbm_default_params(&prm);
        Mat disp(lImg.rows, lImg.cols, kDisp16S);
        if (disp.elemSize() != 2)
            throw std::runtime_error("stereoMatch: this Mat type has no 16-bit elements");
        if (BM_FLAG) {
            bmMatch(disp);
            return disp;
        }
        if (WLS_FLAG) {
            wlsMatch(prm, disp);
            return disp;
        }
        check(svo_sgbm_compute(ctx(), &prm, lImg.data, rImg.data, lImg.cols, lImg.rows, 3, 1,
                               reinterpret_cast<int16_t *>(disp.data), SVO_MEM_HOST));
        return disp;
    }
    // src/StereoCV.cpp:25-28,51-59, commented out upstream: createDisparityWLSFilter(matcher), createRightMatcher(matcher),
    // right_matcher->compute(grayIm2, grayIm1, rdisp), setLambda(lambda), setSigmaColor(sigma), filter(disp, grayIm1, filtDisp,
    // rdisp).  WLS_FLAG = true (opt-in): stereoMatch returns filtDisp (svo_sgbm_wls_compute) and leaves getConfidenceMap()'s
    // values (CV_32F, conf x 255) in confidenceMap.  lambda and sigma are the reference's own.
    bool WLS_FLAG = false;
    double lambda = 400, sigma = 0.4;
    Mat confidenceMap;
    // BM_FLAG = true (opt-in): stereoMatch matches with cv::StereoBM's block matcher (svo_bm_compute; with WLS_FLAG also set,
    // svo_bm_wls_compute) in StereoSGBM's place: the same output format at a fraction of the cost.  bmParams: the disparity
    // range and the speckle filter of the reference's SGBM call (1, 96; 3000, 5), every other field StereoBM::create(0, 21)'s.
    bool BM_FLAG = false;
    svo_bm_params bmParams = bm_defaults();
    static svo_bm_params bm_defaults()
    {
        svo_bm_params p;
        svo_bm_default_params(&p);
        p.min_disparity = 1;
        p.num_disparities = 96;
        p.speckle_window_size = 3000;
        p.speckle_range = 5;
        return p;
    }

    // src/StereoCV.cpp:227-250: Q from stereoRectify, reprojectImageTo3D, points with Z > 5 or Z <= 0.01 skipped,
    // (X, -Y, Z) and lImg's B, G, R as floats in row-major order
    void reprojectDisparity(Mat disp, std::vector<Point3f> &reproject3dPoints, std::vector<Point3f> &colorMap)
    {
        reproject3dPoints.clear();
        colorMap.clear();
        if (disp.empty())
            return;
        if (disp.elemSize() != 2 || lImg.empty() || lImg.rows != disp.rows || lImg.cols != disp.cols)
            throw std::invalid_argument("reprojectDisparity: expected a CV_16S disparity map of lImg's size");
        double Q[16];
        // the rig's own Q (svo_stereo_rectify) is the conventional, metric one: it takes disparities / 16 whatever metricDisparity says
        const bool metric = metricDisparity || RECTIFY_FLAG;
        if (RECTIFY_FLAG) {
            ensureMaps(disp.cols, disp.rows);
            for (int i = 0; i < 16; i++)
                Q[i] = rectQ[i];
        } else {
            check(svo_stereo_rectify_q(focal_x, focal_y, cx, cy, metricDisparity ? -baseline : baseline, disp.cols, disp.rows, Q));
        }
        const size_t n = (size_t)disp.rows * disp.cols;
        std::vector<float> xyz(n * 3), bgr(n * 3);
        int kept = 0;
        check(svo_stereo_reproject(ctx(), reinterpret_cast<const int16_t *>(disp.data), lImg.data, disp.cols, disp.rows,
                                   lImg.channels(), Q, metric ? 1.0f / 16 : 1.0f, 0.01f, 5.0f, 1, xyz.data(),
                                   bgr.data(), &kept, SVO_MEM_HOST));
        reproject3dPoints.reserve(kept);
        colorMap.reserve(kept);
        for (int i = 0; i < kept; i++) {
            reproject3dPoints.emplace_back(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
            colorMap.emplace_back(bgr[3 * i], bgr[3 * i + 1], bgr[3 * i + 2]);
        }
    }

    // src/StereoCV.cpp:275-296 minus ROS: every point in PCL's frame, (x, z, y) x mulFactor 5 (float products), its
    // colour as the uint8_t r = colorMap.z, g = .y, b = .x fields (clamped to 0..255, truncated), then
    // pcl::StatisticalOutlierRemoval with MeanK 20 and StddevMulThresh 0.8 (svo_sor_filter_large, at most 2^22
    // points).  The kept points (x, y, z) and colours (r, g, b) go to publishedCloud / publishedColors, in input order;
    // pts3d and colorMap are left as they are.  voxelLeaf > 0 (ours, opt-in; 0, the default, changes nothing): the converted cloud
    // first goes through voxelDownSample's filter at that leaf, in PCL's frame and units.
    std::vector<Point3f> publishedCloud, publishedColors;
    double voxelLeaf = 0;
    // Open3D's voxel_down_sample (svo_voxel_downsample): pts and colours are REPLACED by one point per
    // occupied voxel of edge `leaf`, the mean of the voxel's points and of their colours, in ascending voxel order.  Points with
    // a non-finite coordinate are dropped.  At most 2^22 points.
    void voxelDownSample(std::vector<Point3f> &pts, std::vector<Point3f> &colours, double leaf)
    {
        if (colours.size() < pts.size())
            throw std::invalid_argument("voxelDownSample: a colour for every point is needed");
        const size_t n = pts.size();
        if (n > (size_t)(1 << 22))
            throw std::length_error("voxelDownSample: at most 2^22 points");
        std::vector<float> xyz(n * 3), bgr(n * 3), xyz_out(n * 3), bgr_out(n * 3);
        for (size_t i = 0; i < n; i++) {
            xyz[3 * i] = pts[i].x, xyz[3 * i + 1] = pts[i].y, xyz[3 * i + 2] = pts[i].z;
            bgr[3 * i] = colours[i].x, bgr[3 * i + 1] = colours[i].y, bgr[3 * i + 2] = colours[i].z;
        }
        int rows = 0;
        check(svo_voxel_downsample(ctx(), xyz.data(), bgr.data(), (int)n, leaf, xyz_out.data(), bgr_out.data(), &rows, nullptr,
                                   nullptr, SVO_MEM_HOST));
        pts.clear();
        colours.clear();
        pts.reserve(rows);
        colours.reserve(rows);
        for (int i = 0; i < rows; i++) {
            pts.emplace_back(xyz_out[3 * i], xyz_out[3 * i + 1], xyz_out[3 * i + 2]);
            colours.emplace_back(bgr_out[3 * i], bgr_out[3 * i + 1], bgr_out[3 * i + 2]);
        }
    }
    void pclPublish(std::vector<Point3f> &pts3d, std::vector<Point3f> &colorMap)
    {
        publishedCloud.clear();
        publishedColors.clear();
        if (colorMap.size() < pts3d.size())
            throw std::invalid_argument("pclPublish: a colour for every point is needed");
        const int mulFactor = 5;
        const size_t n = pts3d.size();
        if (n > (size_t)(1 << 22))
            throw std::length_error("pclPublish: at most 2^22 points");
        std::vector<float> xyz(n * 3), rgb(n * 3), xyz_out(n * 3), rgb_out(n * 3);
        for (size_t i = 0; i < n; i++) {
            xyz[3 * i] = pts3d[i].x * mulFactor;
            xyz[3 * i + 1] = pts3d[i].z * mulFactor;
            xyz[3 * i + 2] = pts3d[i].y * mulFactor;
            rgb[3 * i] = pcl_channel(colorMap[i].z);
            rgb[3 * i + 1] = pcl_channel(colorMap[i].y);
            rgb[3 * i + 2] = pcl_channel(colorMap[i].x);
        }
        int n_sor = (int)n;
        if (voxelLeaf > 0 && n > 0) {  // the voxel grid every PCL pipeline puts in front of the outlier removal: opt-in
            check(svo_voxel_downsample(ctx(), xyz.data(), rgb.data(), (int)n, voxelLeaf, xyz_out.data(), rgb_out.data(), &n_sor,
                                       nullptr, nullptr, SVO_MEM_HOST));
            xyz.swap(xyz_out);
            rgb.swap(rgb_out);
        }
        int kept = 0;
        check(svo_sor_filter_large(ctx(), xyz.data(), rgb.data(), n_sor, 20, 0.8, 0.0f, xyz_out.data(), rgb_out.data(),
                                   &kept, nullptr, nullptr, SVO_MEM_HOST));
        publishedCloud.reserve(kept);
        publishedColors.reserve(kept);
        for (int i = 0; i < kept; i++) {
            publishedCloud.emplace_back(xyz_out[3 * i], xyz_out[3 * i + 1], xyz_out[3 * i + 2]);
            publishedColors.emplace_back(rgb_out[3 * i], rgb_out[3 * i + 1], rgb_out[3 * i + 2]);
        }
    }

    // include/stereoCV.h:62.  The reference pairs SIFT key points by their BRIEF descriptors here (src/StereoCV.cpp:64-121); by
    // default (BRIEF_FLAG = false) this adaptor uses the hot path's dense-grid LK + F-RANSAC + DLT triangulation instead and
    // says so: same output contract (camera-frame 3-D points, colours in color3dMap).
    //
    // BRIEF_FLAG = true (opt-in): the reference's own sequence -- SIFT::create(20000)->detect on both images in one
    // svo_sift_extract_batch call (no SIFT descriptors), BriefDescriptorExtractor::create()->compute on both in one
    // svo_brief_describe_batch call (key points runByImageBorder(28) removes are dropped, as cv erases them),
    // desc.convertTo(CV_32F) + BFMatcher().knnMatch(2) = svo_knn_match(SVO_MATCH_L2_U8, dim briefBytes, k 2), the 0.8 ratio test =
    // svo_ratio_pairs, FmatThresholding (3 px, 0.99) and svo_triangulate with P1 = K[I|0], P2 = K[I|(-baseline, 0, 0)].  The pairs
    // after the ratio test stay in stereoPairs1 / 2, the F-inliers in stereoInliers1 / 2.  Fewer than 8 pairs after the ratio test
    // give an empty out3d.  color3dMap is gathered at the left inliers so that it stays parallel to tri3dPoints, this adaptor's
    // contract; upstream leaves color3dMap alone in this method.  The test table is the library's own unless
    // svo_brief_set_pattern has set OpenCV's.
    bool BRIEF_FLAG = false;
    // ours, opt-in (off: every method issues the calls it always issued): with BRIEF_FLAG / SIFT_FLAG, CROSS_CHECK_FLAG pairs the
    // features by svo_match_cross(SVO_CROSS_CV) -- BFMatcher(norm, true).match -- instead of knnMatch(2) + ratio 0.8;
    // EPIPOLAR_GATE_FLAG restricts stereoTriangulate's candidates to the right features within epipolarRows rows of the left one
    // and 0 ... maxDisparity columns to its left (svo_knn_match_gated; the pair is taken as rectified)
    bool CROSS_CHECK_FLAG = false;
    bool EPIPOLAR_GATE_FLAG = false;
    float epipolarRows = 2.0f;
    float maxDisparity = 128.0f;
    int siftFeaturesStereo = 20000, briefBytes = 32;
    std::vector<Point2f> stereoPairs1, stereoPairs2, stereoInliers1, stereoInliers2;

    // A raw rig (ours, opt-in; RECTIFY_FLAG = false, the default, changes nothing): setCalibration takes both cameras' K (9) and
    // D (0, 4, 5 or 8 coefficients) and the pose of camera 1 in camera 2, x2 = R x1 + T (9, 3).  With RECTIFY_FLAG set,
    // stereoMatch, stereoTriangulate and monocularTriangulate see images that went through svo_rectify_pairs (cv::stereoRectify
    // with CALIB_ZERO_DISPARITY and alpha = -1 -> initUndistortRectifyMap -> remap; the maps are built at
    // the first frame's size and kept), and reprojectDisparity takes Q from svo_stereo_rectify with disparities / 16 (that Q is metric,
    // so metricDisparity is implied).  rectR1 ... rectQ hold the
    // rectification once a frame was seen.  The intrinsics the triangulation uses (focal_x, cx, ..., baseline) stay the caller's to
    // set: rectP1 / rectP2 hold the rectified ones.
    bool RECTIFY_FLAG = false;
    double rectR1[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, rectR2[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, rectP1[12] = {0}, rectP2[12] = {0},
           rectQ[16] = {0};
    void setCalibration(const std::vector<double> &K1, const std::vector<double> &D1, const std::vector<double> &K2,
                        const std::vector<double> &D2, const std::vector<double> &R, const std::vector<double> &T)
    {
        if (K1.size() != 9 || K2.size() != 9 || R.size() != 9 || T.size() != 3)
            throw std::invalid_argument("setCalibration: K1, K2 and R hold 9 numbers, T holds 3");
        calK1_ = K1, calD1_ = D1, calK2_ = K2, calD2_ = D2, calR_ = R, calT_ = T;
        mapL_.reset();
        mapR_.reset();
        mapW_ = mapH_ = 0;
    }
    // cv::undistortPoints(pts, K, D, R_i, P_i) of one camera of the rig (svo_undistort_points): raw pixels -> rectified pixels.
    // width x height: the frame size the rectification is computed for.
    void undistortPoints(const std::vector<Point2f> &pts, std::vector<Point2f> &out, int width, int height, bool rightCamera = false)
    {
        ensureMaps(width, height);
        out.assign(pts.size(), Point2f());
        const std::vector<double> &K = rightCamera ? calK2_ : calK1_, &D = rightCamera ? calD2_ : calD1_;
        check(svo_undistort_points(ctx(), fp(pts), (int)pts.size(), K.data(), D.empty() ? nullptr : D.data(), (int)D.size(),
                                   rightCamera ? rectR2 : rectR1, rightCamera ? rectP2 : rectP1,
                                   reinterpret_cast<float *>(out.data()), SVO_MEM_HOST));
    }
    // both images of a pair through the rig's maps; sameCamera: both are the LEFT camera's (monocularTriangulate)
    void rectifyPair(const Mat &im1, const Mat &im2, Mat &out1, Mat &out2, bool sameCamera)
    {
        const int w = mat_cols(im1), h = mat_rows(im1), c = mat_channels(im1);
        if (mat_data(im1) == nullptr || mat_data(im2) == nullptr || mat_cols(im2) != w || mat_rows(im2) != h || mat_channels(im2) != c)
            throw std::invalid_argument("rectifyPair: two images of one size are needed");
        ensureMaps(w, h);
        out1 = Mat(h, w, im1.type());
        out2 = Mat(h, w, im2.type());
        check(svo_rectify_pairs(ctx(), mapL_.get(), sameCamera ? mapL_.get() : mapR_.get(), mat_data(im1), mat_data(im2), 1, c, 0,
                                out1.data, out2.data, SVO_MEM_HOST));
    }
    void stereoTriangulate(const Mat &raw1, const Mat &raw2, std::vector<Point3f> &out3d)
    {
        Mat rect1, rect2;
        if (RECTIFY_FLAG)
            rectifyPair(raw1, raw2, rect1, rect2, false);
        const Mat &im1 = RECTIFY_FLAG ? rect1 : raw1, &im2 = RECTIFY_FLAG ? rect2 : raw2;
        slam_.baseline = baseline;
        slam_.focal_x = focal_x;
        slam_.focal_y = focal_y;
        slam_.cx = cx;
        slam_.cy = cy;
        if (BRIEF_FLAG) {
            briefStereoTriangulate(im1, im2, out3d);
            return;
        }
        std::vector<Point2f> pts2d;
        slam_.stereoTriangulate(im1, im2, out3d, pts2d);
        tri3dPoints = out3d;
        color3dMap = slam_.colors;
    }
    // brief->compute(img, keypoints, desc) on one image: the key points runByImageBorder(28) removes are erased from
    // `keypoints`, desc holds briefBytes bytes per remaining key point
    void briefFeatures(const Mat &img, std::vector<KeyPoint> &keypoints, std::vector<uint8_t> &desc)
    {
        const Mat *imgs[1] = {&img};
        std::vector<uint8_t> d[1];
        briefFeaturesBatch(imgs, 1, &keypoints, d);
        desc.swap(d[0]);
    }

    // include/stereoCV.h:66, src/StereoCV.cpp:123-188: two-view monocular reconstruction.  The reference matches SIFT
    // features with a ratio test here; by default (SIFT_FLAG = false) this adaptor uses the hot path's dense grid + LK
    // instead, as stereoTriangulate does: denseKeypointExtractor / denseLKtracking(im1 -> im2) / FmatThresholding (3 px, 0.99), then
    // svo_find_essential (1 px, 0.99) and svo_recover_pose on the F-inliers, and svo_triangulate of ALL F-inliers (as
    // upstream: inlier1 / inlier2, not the E inliers) with P1 = K[I|0], P2 = K[R|t] -- float points, t of unit norm.
    // The pose lands in monoR / monoT, the F-inliers in monoPts1 / monoPts2.
    //
    // SIFT_FLAG = true (opt-in): the reference's own sequence instead of the grid + LK -- SIFT::create(10000) on both images
    // in one svo_sift_extract_batch call, BFMatcher().knnMatch(desc1, desc2, 2) = svo_knn_match(SVO_MATCH_L2_F32, k 2), the
    // 0.8 ratio test = svo_ratio_pairs, then FmatThresholding and the same tail.  siftCapacity bounds the key points an
    // image may return (retainBest keeps ties, so it can exceed the budget); beyond it the call throws SVO_ERR_CAPACITY.
    //
    // HOMOGRAPHY_FLAG = true (opt-in): for a scene that is one plane (a road, a wall at a loop closure), where F and E are
    // degenerate, or for a pure rotation -- after the F filter, svo_find_homography (homographyThreshold px, 0.995, 2000)
    // in findEssentialMat's place and svo_homography_pose in recoverPose's; the plane's unit normal (first camera's frame)
    // lands in planeNormal; a pure rotation gives monoT = 0.  The rest of the member is unchanged.
    double monoR[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, monoT[3] = {0, 0, 0};
    std::vector<Point2f> monoPts1, monoPts2;
    bool HOMOGRAPHY_FLAG = false;
    double homographyThreshold = 3.0;
    double planeNormal[3] = {0, 0, 0};
    bool SIFT_FLAG = false;
    int siftFeaturesMono = 10000, siftCapacity = 40000;
    // detector->detect + compute of SIFT::create(nfeatures) on one image: KeyPoint fields as cv fills them, desc: 128
    // floats per key point (what desc.convertTo(CV_32F) holds)
    void siftFeatures(const Mat &img, std::vector<KeyPoint> &kps, std::vector<float> &desc, int nfeatures)
    {
        const Mat *imgs[1] = {&img};
        std::vector<KeyPoint> k[1];
        std::vector<float> d[1];
        siftFeaturesBatch(imgs, 1, nfeatures, k, d);
        kps.swap(k[0]);
        desc.swap(d[0]);
    }
    void monocularTriangulate(const Mat &raw1, const Mat &raw2, std::vector<Point3f> &out3d)
    {
        Mat rect1, rect2;
        if (RECTIFY_FLAG)
            rectifyPair(raw1, raw2, rect1, rect2, true);
        const Mat &im1 = RECTIFY_FLAG ? rect1 : raw1, &im2 = RECTIFY_FLAG ? rect2 : raw2;
        std::vector<Point2f> pt1, pt2;
        if (SIFT_FLAG) {
            siftRatioPairs(im1, im2, pt1, pt2);
        } else {
            std::vector<KeyPoint> dkps = slam_.denseKeypointExtractor(im1, slam_.gridStep);
            for (const KeyPoint &k : dkps)
                pt1.emplace_back(k.pt);
            slam_.denseLKtracking(im1, im2, pt1, pt2);
        }
        slam_.FmatThresholding(pt1, pt2);
        monoPts1 = pt1;
        monoPts2 = pt2;
        const int n = (int)pt1.size();
        const int offsets[2] = {0, n};
        const double K4[4] = {focal_x, focal_y, cx, cy};
        std::vector<uint8_t> mask(n > 0 ? n : 1);
        if (HOMOGRAPHY_FLAG) {
            double H[9];
            int count = 0;
            check(svo_find_homography(ctx(), fp(pt1), fp(pt2), offsets, 1, homographyThreshold, 0.995, 2000, slam_.ransacSeed + 4,
                                      mask.data(), H, &count, nullptr, SVO_MEM_HOST));
            if (count < 4)
                throw std::runtime_error("monocularTriangulate: no homography");
            check(svo_homography_pose(ctx(), H, fp(pt1), fp(pt2), offsets, 1, K4, 50.0, nullptr, monoR, monoT, planeNormal, nullptr,
                                      SVO_MEM_HOST));
        } else {
            double E[90];
            int nmodels = 0;
            check(svo_find_essential(ctx(), fp(pt1), fp(pt2), offsets, 1, K4, 1.0, 0.99, 1000, slam_.ransacSeed + 4, mask.data(),
                                     E, &nmodels, nullptr, nullptr, SVO_MEM_HOST));
            if (nmodels < 1)
                throw std::runtime_error("monocularTriangulate: no essential matrix");
            int good = 0;
            check(svo_recover_pose(ctx(), E, fp(pt1), fp(pt2), offsets, 1, K4, 50.0, nullptr, monoR, monoT, &good, SVO_MEM_HOST));
        }
        const double K[9] = {focal_x, 0, cx, 0, focal_y, cy, 0, 0, 1};
        double P1[12], P2[12];
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 4; c++) {
                P1[4 * r + c] = c < 3 ? K[3 * r + c] : 0.;
                double s = 0;
                for (int k = 0; k < 3; k++)
                    s += K[3 * r + k] * (c < 3 ? monoR[3 * k + c] : monoT[k]);
                P2[4 * r + c] = s;
            }
        out3d.assign(n, Point3f());
        if (n > 0)
            check(svo_triangulate(ctx(), P1, P2, fp(pt1), fp(pt2), n, reinterpret_cast<float *>(out3d.data()), nullptr,
                                  SVO_MEM_HOST));
    }

    // include/stereoCV.h:60 (private upstream): a frame as stereoMatch loads it, B,G,R; empty when it is missing
    Mat getImg(const char *pattern, int iter) { return load_bgr(pattern, iter); }

  private:
    static const float *fp(const std::vector<Point2f> &v) { return reinterpret_cast<const float *>(v.data()); }
    std::vector<double> calK1_, calD1_, calK2_, calD2_, calR_, calT_;
    std::shared_ptr<svo_rectify_map> mapL_, mapR_;
    int mapW_ = 0, mapH_ = 0;
    // the rectification and both maps for frames of w x h, built once per size
    void ensureMaps(int w, int h)
    {
        if (calK1_.empty())
            throw std::logic_error("RECTIFY_FLAG / undistortPoints: setCalibration has not been called");
        if (mapL_ && mapR_ && mapW_ == w && mapH_ == h)
            return;
        const double *d1 = calD1_.empty() ? nullptr : calD1_.data(), *d2 = calD2_.empty() ? nullptr : calD2_.data();
        check(svo_stereo_rectify(calK1_.data(), d1, (int)calD1_.size(), calK2_.data(), d2, (int)calD2_.size(), w, h, calR_.data(),
                                 calT_.data(), SVO_CALIB_ZERO_DISPARITY, -1.0, 0, 0, rectR1, rectR2, rectP1, rectP2, rectQ));
        svo_ctx *c = ctx();
        svo_rectify_map *l = nullptr, *r = nullptr;
        check(svo_rectify_map_create(c, calK1_.data(), d1, (int)calD1_.size(), rectR1, rectP1, w, h, w, h, &l));
        mapL_.reset(l, [c](svo_rectify_map *m) { svo_rectify_map_destroy(c, m); });
        check(svo_rectify_map_create(c, calK2_.data(), d2, (int)calD2_.size(), rectR2, rectP2, w, h, w, h, &r));
        mapR_.reset(r, [c](svo_rectify_map *m) { svo_rectify_map_destroy(c, m); });
        mapW_ = w, mapH_ = h;
    }
    // n images of one size through one svo_sift_extract_batch call
    // (desc == nullptr: detect only)
    void siftFeaturesBatch(const Mat *const *imgs, int n, int nfeatures, std::vector<KeyPoint> *kps, std::vector<float> *desc)
    {
        const uint8_t *ptrs[16];
        same_size_ptrs(imgs, n, "siftFeatures", ptrs);
        const Mat &first = *imgs[0];
        svo_sift_params prm;
        svo_sift_default_params(&prm);
        prm.n_features = nfeatures;
        const size_t cap = (size_t)(siftCapacity > 0 ? siftCapacity : 1), e = cap * (size_t)n;
        std::vector<float> xy(2 * e), size(e), angle(e), resp(e), d(desc ? 128 * e : 0);
        std::vector<int> oct(e), cnt((size_t)n);
        check(svo_sift_extract_batch(ctx(), ptrs, n, mat_cols(first), mat_rows(first), mat_channels(first), &prm, (int)cap,
                                     xy.data(), size.data(), angle.data(), resp.data(), oct.data(), desc ? d.data() : nullptr, cnt.data(),
                                     SVO_MEM_HOST));
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
            }
            if (desc)
                desc[i].assign(d.begin() + 128 * b, d.begin() + 128 * (b + m));
        }
    }
    // n images of one size through one svo_brief_describe_batch call; kps[i] loses the key points the border filter removes
    void briefFeaturesBatch(const Mat *const *imgs, int n, std::vector<KeyPoint> *kps, std::vector<uint8_t> *desc)
    {
        const uint8_t *ptrs[16];
        same_size_ptrs(imgs, n, "briefFeatures", ptrs);
        const Mat &first = *imgs[0];
        size_t cap = 1;
        for (int i = 0; i < n; i++)
            cap = kps[i].size() > cap ? kps[i].size() : cap;
        const size_t nb = (size_t)briefBytes, e = cap * (size_t)n;
        std::vector<float> xy(2 * e);
        std::vector<int> n_in((size_t)n), n_out((size_t)n), kept(e);
        std::vector<uint8_t> d(e * (nb > 0 ? nb : 1));
        for (int i = 0; i < n; i++) {
            n_in[(size_t)i] = (int)kps[i].size();
            for (size_t j = 0; j < kps[i].size(); j++) {
                xy[2 * (cap * i + j)] = kps[i][j].pt.x;
                xy[2 * (cap * i + j) + 1] = kps[i][j].pt.y;
            }
        }
        check(svo_brief_describe_batch(ctx(), ptrs, n, mat_cols(first), mat_rows(first), mat_channels(first), briefBytes, xy.data(),
                                       n_in.data(), (int)cap, kept.data(), d.data(), n_out.data(), SVO_MEM_HOST));
        for (int i = 0; i < n; i++) {
            const size_t b = cap * (size_t)i, m = (size_t)n_out[(size_t)i];
            std::vector<KeyPoint> stay(m);
            for (size_t j = 0; j < m; j++)
                stay[j] = kps[i][(size_t)kept[b + j]];
            kps[i].swap(stay);
            desc[i].assign(d.begin() + nb * b, d.begin() + nb * (b + m));
        }
    }
    // src/StereoCV.cpp:64-121
    void briefStereoTriangulate(const Mat &im1, const Mat &im2, std::vector<Point3f> &out3d)
    {
        out3d.clear();
        tri3dPoints.clear();
        color3dMap.clear();
        stereoPairs1.clear();
        stereoPairs2.clear();
        stereoInliers1.clear();
        stereoInliers2.clear();
        const Mat *imgs[2] = {&im1, &im2};
        std::vector<KeyPoint> kps[2];
        siftFeaturesBatch(imgs, 2, siftFeaturesStereo, kps, nullptr);
        std::vector<uint8_t> desc[2];
        briefFeaturesBatch(imgs, 2, kps, desc);
        const std::vector<Point2f> xy1 = keypoint_points(kps[0]), xy2 = keypoint_points(kps[1]);
        std::vector<Point2f> pt1, pt2;
        sparse_match_points(ctx(), SparseMatch{CROSS_CHECK_FLAG, EPIPOLAR_GATE_FLAG, epipolarRows, maxDisparity}, SVO_MATCH_L2_U8,
                            desc[0].data(), desc[1].data(), briefBytes, (int)xy1.size(), (int)xy2.size(), fp(xy1), fp(xy2), pt1, pt2);
        stereoPairs1 = pt1;
        stereoPairs2 = pt2;
        if (pt1.size() < 8)
            return;
        slam_.FmatThresholding(pt1, pt2);
        stereoInliers1 = pt1;
        stereoInliers2 = pt2;
        const int n = (int)pt1.size();
        if (n == 0)
            return;
        double P1[12], P2[12];
        check(svo_stereo_projections(focal_x, focal_y, cx, cy, baseline, P1, P2));
        out3d.assign((size_t)n, Point3f());
        check(svo_triangulate(ctx(), P1, P2, fp(pt1), fp(pt2), n, reinterpret_cast<float *>(out3d.data()), nullptr, SVO_MEM_HOST));
        // getColors(im1, inlier1), include/monoUtils.h:180-193
        color3dMap.assign((size_t)n, Point3f());
        svo_pyramid *p = nullptr;
        check(svo_pyramid_create(ctx(), mat_cols(im1), mat_rows(im1), mat_channels(im1), 1, &p));
        int rc = svo_pyramid_build(ctx(), p, mat_data(im1), SVO_MEM_HOST);
        if (rc == SVO_OK)
            rc = svo_get_colors(ctx(), p, fp(pt1), n, reinterpret_cast<float *>(color3dMap.data()), SVO_MEM_HOST);
        svo_pyramid_destroy(ctx(), p);
        check(rc);
        tri3dPoints = out3d;
    }
    void bmMatch(Mat &disp)
    {
        int16_t *out = reinterpret_cast<int16_t *>(disp.data);
        if (!WLS_FLAG) {
            check(svo_bm_compute(ctx(), &bmParams, lImg.data, rImg.data, lImg.cols, lImg.rows, 3, 1, out, SVO_MEM_HOST));
            return;
        }
        svo_wls_params wls;
        svo_wls_default_params_bm(&bmParams, &wls);
        wls.lambda = lambda;
        wls.sigma_color = sigma;
        confidenceMap = Mat(lImg.rows, lImg.cols, kConf32F);
        if (confidenceMap.elemSize() != 4)
            throw std::runtime_error("stereoMatch: this Mat type has no 32-bit float elements");
        check(svo_bm_wls_compute(ctx(), &bmParams, &wls, lImg.data, rImg.data, lImg.cols, lImg.rows, 3, 1, out, nullptr, nullptr,
                                 reinterpret_cast<float *>(confidenceMap.data), SVO_MEM_HOST));
    }
    void wlsMatch(const svo_sgbm_params &prm, Mat &disp)
    {
        svo_wls_params wls;
        svo_wls_default_params(&prm, &wls);
        wls.lambda = lambda;
        wls.sigma_color = sigma;
        confidenceMap = Mat(lImg.rows, lImg.cols, kConf32F);
        if (confidenceMap.elemSize() != 4)
            throw std::runtime_error("stereoMatch: this Mat type has no 32-bit float elements");
        check(svo_sgbm_wls_compute(ctx(), &prm, &wls, lImg.data, rImg.data, lImg.cols, lImg.rows, 3, 1,
                                   reinterpret_cast<int16_t *>(disp.data), nullptr, nullptr,
                                   reinterpret_cast<float *>(confidenceMap.data), SVO_MEM_HOST));
    }
    // src/StereoCV.cpp:123-147: SIFT(10000) on both images, knnMatch(desc1, desc2, 2), m.distance < 0.8 * n.distance
    void siftRatioPairs(const Mat &im1, const Mat &im2, std::vector<Point2f> &pt1, std::vector<Point2f> &pt2)
    {
        const Mat *imgs[2] = {&im1, &im2};
        std::vector<KeyPoint> kps[2];
        std::vector<float> desc[2];
        siftFeaturesBatch(imgs, 2, siftFeaturesMono, kps, desc);
        const std::vector<Point2f> xy1 = keypoint_points(kps[0]), xy2 = keypoint_points(kps[1]);
        // two views of one camera: no epipolar rows to gate by
        sparse_match_points(ctx(), SparseMatch{CROSS_CHECK_FLAG, false, epipolarRows, maxDisparity}, SVO_MATCH_L2_F32, desc[0].data(),
                            desc[1].data(), 128, (int)xy1.size(), (int)xy2.size(), fp(xy1), fp(xy2), pt1, pt2);
    }
#if defined(SVO_WITH_OPENCV) && defined(CV_16SC1)
    static constexpr int kDisp16S = CV_16SC1;
#else
    static constexpr int kDisp16S = 3;  // CV_16SC1
#endif
#if defined(SVO_WITH_OPENCV) && defined(CV_32FC1)
    static constexpr int kConf32F = CV_32FC1;
#else
    static constexpr int kConf32F = 5;  // CV_32FC1
#endif
    svo_ctx *ctx_ = nullptr;
    // a float colour as a uint8_t field of pcl::PointXYZRGB holds it: clamped to 0..255 (NaN to 0), then truncated
    static float pcl_channel(float v) { return v > 0.f ? (float)(uint8_t)(v < 255.f ? v : 255.f) : 0.f; }
    svo_ctx *ctx() { return ctx_ ? ctx_ : (ctx_ = shared_context()); }
    static Mat k_matrix(double fx, double fy, double cx_, double cy_)
    {
        Mat k = Mat::zeros(3, 3, CV_64F);
        k.at<double>(0, 0) = fx, k.at<double>(0, 2) = cx_, k.at<double>(1, 1) = fy, k.at<double>(1, 2) = cy_;
        k.at<double>(2, 2) = 1;
        return k;
    }
    static Mat load_bgr(const char *pattern, int iter)
    {
        char path[1024];
        int w = 0, h = 0, c = 0;
        if (!pattern || svo_io_format_path(path, (int)sizeof(path), pattern, iter) != SVO_OK ||
            svo_io_image_info(path, &w, &h, &c) != SVO_OK) {
            std::fprintf(stderr, "\n\nYIKES Dawg, Failed to fetch frame, check the file path\n\n\n");
            return Mat();
        }
        Mat im(h, w, CV_8UC3);
        if (svo_io_read_image(path, 3, im.data, (size_t)w * h * 3, &w, &h) != SVO_OK)
            return Mat();
        return im;
    }
    visualSLAM slam_;
};

}  // namespace svo_compat
