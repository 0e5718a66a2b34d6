// svo_compat/visualSLAM.hpp -- the hot-path member surface of the reference's visualSLAM
// class (include/visualSLAM.h:152-178) on top of the svo_* C ABI.
//
// Two levels, same results:
//  * stage methods with the reference's names and argument meaning (denseKeypointExtractor,
//    denseLKtracking, FmatThresholding, stereoTriangulate, PyrLKtrackFrame2Frame,
//    insertKeyFrames, update3dtransformation, PerspectiveNpointEstimation, stageForPGO,
//    updateOdometry).  Containers are the caller's, outputs are cleared and refilled through
//    references, the side-channel members (colors, untransformed, inlierReferencePyrLKPts,
//    refDrawPts, trackedDrawPts, referenceImg, currentImage, LC_FLAG, LCidx, cooldownTimer,
//    SHUTDOWN_FLAG) behave as in the reference.  Each call stages its host containers
//    through the device (like the reference, it rebuilds image pyramids per call).
//  * processFrame(): the body of initSequence's loop (src/VisualSLAM.cpp:54-169) on the
//    fused, device-resident front-end (svo_vo) + the device pose graph -- the fast path.
//  * SORcloud(): the map clean-up of src/rosFuncs.cpp:9-39 (PCL StatisticalOutlierRemoval) on the GPU.
//  * checkLoopDetectorStatus(): src/optimizationStuff.cpp:49-64 on the GPU (svo_lc); processFrame
//    still takes the match as an argument so that a caller may keep its own detector.
// Not here (out of the hot path): ROS publishing, Pangolin viewer.
#pragma once

#include <cstdio>

#include "poseGraph.hpp"
#include "surf.hpp"
#include "types.hpp"

namespace svo_compat {

struct keyFrame {  // include/visualSLAM.h:47-54
    int idx = -1;
    bool retrack = false;
    Mat33d R;
    Vec3d t;
    std::vector<Point3f> ref3dCoords;
};

class visualSLAM {
  public:
    // ---- public state of the reference (include/visualSLAM.h:66-113) ----
    double baseline = 0.54;
    int LCidx = 0;
    int cooldownTimer = 0;
    bool LC_FLAG = false;
    bool SHUTDOWN_FLAG = false;
    // true: the dense grid + LK branch of stereoTriangulate; false: its ORB + BFMatcher branch (src/triangulation.cpp:104-134).
    // Only the stage method reads it: processFrame's fused svo_vo_* runner is dense-only.
    bool DENSE_FLAG = true;
    int orbFeatures = 1000;         // ORB::create(1000), src/triangulation.cpp:105
    // with DENSE_FLAG == false: true = the sparse branch as include/trangulation.h:32-61 writes it, SURF::create(surfHessian)
    // in ORB's place
    bool SURF_FLAG = false;
    int surfHessian = 1200;
    // with DENSE_FLAG == true: true = the reference points of stereoTriangulate come from fastKeypointExtractor (cv::FAST as the
    // demo of src/ANMS.cpp:76 calls it, threshold 1) instead of the grid; fastKeep > 0 passes them through
    // adaptiveNonMaximalSuppresion(kps, fastKeep) (src/ANMS.cpp:18-67) on the device.  Off: every method issues the calls it
    // always issued.
    bool FAST_FLAG = false;
    int fastThreshold = 1;
    int fastKeep = 0;
    // with DENSE_FLAG == true and FAST_FLAG == false: true = the reference points of stereoTriangulate come from
    // gfttKeypointExtractor (cv::goodFeaturesToTrack: Shi-Tomasi corners, the measure LK's own minEigThreshold test uses) instead
    // of the grid.  Off: every method issues the calls it always issued.
    bool GFTT_FLAG = false;
    int gfttMaxCorners = 1000;
    double gfttQuality = 0.01;
    double gfttMinDistance = 10;
    // with DENSE_FLAG == false and SURF_FLAG == false: true = the sparse branch with the commented detector / descriptor pair of
    // src/triangulation.cpp:79-80, StarDetector::create() (starMaxSize, starResponseThreshold; the other arguments at their
    // defaults) + BriefDescriptorExtractor::create(), in ORB's place.  Off: every method issues the calls it always issued.
    bool STAR_FLAG = false;
    int starMaxSize = 45;
    int starResponseThreshold = 30;
    // with DENSE_FLAG == false (ours, opt-in; off: every method issues the calls it always issued): CROSS_CHECK_FLAG pairs the
    // features of every sparse branch by svo_match_cross(SVO_CROSS_CV) -- BFMatcher(norm, true).match -- instead of knnMatch(2) +
    // ratio 0.8; EPIPOLAR_GATE_FLAG restricts a left feature's candidates to the right features within epipolarRows rows of it
    // and 0 ... maxDisparity columns to its left (svo_knn_match_gated; the pair is taken as rectified)
    bool CROSS_CHECK_FLAG = false;
    bool EPIPOLAR_GATE_FLAG = false;
    float epipolarRows = 2.0f;
    float maxDisparity = 128.0f;
    SparseMatch sparseMatch() const { return SparseMatch{CROSS_CHECK_FLAG, EPIPOLAR_GATE_FLAG, epipolarRows, maxDisparity}; }
    double focal_x = 7.188560000000e+02, cx = 6.071928000000e+02;
    double focal_y = 7.188560000000e+02, cy = 1.852157000000e+02;
    int gridStep = 30;              // src/triangulation.cpp:89
    int keyframeMinInliers = 200;   // src/VisualSLAM.cpp:120
    int loopMinGap = 100;           // query - match > 100, src/optimizationStuff.cpp:58
    int loopCooldown = 100;         // cooldownTimer = 100, src/optimizationStuff.cpp:62
    bool mapSOR = true;             // SORcloud(untransformed, colors) before a record is stored, src/VisualSLAM.cpp:154
    uint64_t ransacSeed = 0;
    Mat referenceImg, currentImage;
    std::vector<Point3f> untransformed, colors;
    std::vector<Point2f> refDrawPts, trackedDrawPts, inlierReferencePyrLKPts;
    std::vector<std::vector<Point3f>> mapHistory, colorHistory;
    std::vector<Vec3d> trajectory;
    std::vector<keyFrame> keyFrameHistory;
    std::vector<Isometry3d> isoVector;
    globalPoseGraph poseGraph;

    explicit visualSLAM(svo_ctx *ctx = nullptr) : poseGraph(ctx ? ctx : shared_context()), ctx_(ctx ? ctx : shared_context()) {}
    ~visualSLAM()
    {
        if (vo_)
            svo_vo_destroy(vo_);
        if (lc_)
            svo_lc_destroy(lc_);
        if (map_)
            svo_map_destroy(map_);
    }
    visualSLAM(const visualSLAM &) = delete;
    visualSLAM &operator=(const visualSLAM &) = delete;

    // ---- src/keyFrameManagement.cpp:48-71: loadImageL / loadImageR = sprintf(FileName, lFptr, iter) + imread(FileName) ----
    // The printf patterns of include/visualSLAM.h:80,116-117 ("<dir>/image_2/%0.6d.png", src/VisualSLAM.cpp:220-222).  The
    // frame is decoded by the library (svo_io_load_frame: PNG -- KITTI's format --, PGM, PPM; no OpenCV imgcodecs needed) into
    // what imread's default flag gives: 8-bit B,G,R interleaved.  A missing or damaged file gives an empty Mat and the
    // reference's message, as upstream (it only prints and carries on).
    const char *lFptr = nullptr, *rFptr = nullptr;
    Mat loadImageL(int iter) { return load_frame(lFptr, iter); }
    Mat loadImageR(int iter) { return load_frame(rFptr, iter); }

    // ---- src/tracking.cpp:4-12 ----
    std::vector<KeyPoint> denseKeypointExtractor(const Mat &img, int stepSize)
    {
        int n = 0;
        check(svo_grid_keypoints(ctx_, mat_rows(img), mat_cols(img), stepSize, nullptr, 0, SVO_MEM_HOST, &n));
        std::vector<float> xy((size_t)n * 2);
        check(svo_grid_keypoints(ctx_, mat_rows(img), mat_cols(img), stepSize, xy.data(), n, SVO_MEM_HOST, &n));
        std::vector<KeyPoint> out;
        out.reserve(n);
        for (int i = 0; i < n; i++)
            out.emplace_back(xy[2 * i], xy[2 * i + 1], (float)stepSize);
        return out;
    }

    // ---- src/ANMS.cpp:69-82: cv::FAST(image, kps, fastThreshold) [-> adaptiveNonMaximalSuppresion(kps, fastKeep)] ----
    // Key points carry their response (the corner score), size 7 and angle -1 as cv::FAST leaves them; row-major order with
    // fastKeep == 0, ANMS's response-sorted order otherwise.
    std::vector<KeyPoint> fastKeypointExtractor(Mat img)
    {
        std::vector<KeyPoint> out;
        if (mat_data(img) == nullptr)
            return out;
        svo_fast_params prm;
        svo_fast_default_params(&prm);
        prm.threshold = fastThreshold;
        const uint8_t *imgs[1] = {mat_data(img)};
        const int w = mat_cols(img), h = mat_rows(img), c = mat_channels(img);
        int cap = 4096, n = 0;
        std::vector<float> xy, resp;
        for (;;) {
            xy.resize((size_t)cap * 2);
            resp.resize((size_t)cap);
            const int rc = fastKeep > 0 ? svo_fast_anms_batch(ctx_, imgs, 1, w, h, c, &prm, fastKeep, cap, xy.data(), resp.data(), &n,
                                                              SVO_MEM_HOST)
                                        : svo_fast_detect_batch(ctx_, imgs, 1, w, h, c, &prm, cap, xy.data(), resp.data(), nullptr, &n,
                                                                SVO_MEM_HOST);
            if (rc != SVO_ERR_CAPACITY)
                check(rc);
            if (rc == SVO_OK)
                break;
            cap = n;  // the needed count
        }
        out.reserve((size_t)n);
        for (int i = 0; i < n; i++) {
            out.emplace_back(xy[2 * (size_t)i], xy[2 * (size_t)i + 1], 7.f);
            out.back().response = resp[(size_t)i];
        }
        return out;
    }

    // ---- cv::goodFeaturesToTrack(img, corners, gfttMaxCorners, gfttQuality, gfttMinDistance) as GFTTDetector::detect returns it ----
    // Key points in acceptance order (measure descending among the accepted) with size = the block size, angle -1 and the
    // measure as response.
    std::vector<KeyPoint> gfttKeypointExtractor(Mat img)
    {
        std::vector<KeyPoint> out;
        if (mat_data(img) == nullptr)
            return out;
        svo_gftt_params prm;
        svo_gftt_default_params(&prm);
        prm.max_corners = gfttMaxCorners;
        prm.quality_level = gfttQuality;
        prm.min_distance = gfttMinDistance;
        const uint8_t *imgs[1] = {mat_data(img)};
        const int w = mat_cols(img), h = mat_rows(img), c = mat_channels(img);
        int cap = gfttMaxCorners > 0 ? gfttMaxCorners : 4096, n = 0;
        std::vector<float> xy, resp;
        for (;;) {
            xy.resize((size_t)cap * 2);
            resp.resize((size_t)cap);
            const int rc = svo_gftt_detect_batch(ctx_, imgs, nullptr, 1, w, h, c, &prm, cap, xy.data(), resp.data(), &n, SVO_MEM_HOST);
            if (rc != SVO_ERR_CAPACITY)
                check(rc);
            if (rc == SVO_OK)
                break;
            cap = n;  // the needed count
        }
        out.reserve((size_t)n);
        for (int i = 0; i < n; i++) {
            out.emplace_back(xy[2 * (size_t)i], xy[2 * (size_t)i + 1], (float)prm.block_size);
            out.back().response = resp[(size_t)i];
        }
        return out;
    }

    // ---- src/triangulation.cpp:79: StarDetector::create(starMaxSize, starResponseThreshold)->detect(img, kps) ----
    // Key points carry their size (the outer size of the winning pattern) and response (negative for dark blobs), angle -1 and
    // octave 0 as the detector leaves them; a tile's maximum before its minimum, tiles in row-major order.
    std::vector<KeyPoint> starKeypointExtractor(Mat img)
    {
        std::vector<KeyPoint> out[1];
        if (mat_data(img) == nullptr)
            return out[0];
        const Mat *imgs[1] = {&img};
        starKeypointsBatch(imgs, 1, out);
        return out[0];
    }

    // ---- include/monoUtils.h:195-213 (declared at include/visualSLAM.h:162) ----
    // The indices of newref2dFeatures, ascending, with no base point listed in `mask` within `radius`: svo_dedup_points in DISC mode.
    // A negative radius keeps everything upstream (no norm is below it); it is passed on as 0, which does too.
    std::vector<int> removeDuplicates(std::vector<Point2f> &baseref2dFeatures, std::vector<Point2f> &newref2dFeatures,
                                      std::vector<int> &mask, int radius = 10)
    {
        return remove_duplicates(ctx_, baseref2dFeatures, newref2dFeatures, mask, radius < 0 ? 0 : radius);
    }

    // ---- src/tracking.cpp:14-28 ----
    void denseLKtracking(const Mat &refImg, const Mat &curImg, std::vector<Point2f> &refPts,
                         std::vector<Point2f> &trackPts)
    {
        std::vector<Point2f> trk(refPts.size());
        std::vector<uint8_t> status(refPts.size());
        lk(refImg, curImg, refPts, trk, status);
        compact2(status, refPts, trk);
        trackPts = trk;
    }

    // ---- src/tracking.cpp:30-43: findFundamentalMat(..., CV_RANSAC, 3.0, 0.99, mask) ----
    void FmatThresholding(std::vector<Point2f> &refPts, std::vector<Point2f> &trkPts)
    {
        std::vector<uint8_t> mask(refPts.size());
        int cnt = 0;
        check(svo_fransac(ctx_, f(refPts), f(trkPts), (int)refPts.size(), 3.0, 0.99, 1000, ransacSeed + 3, mask.data(),
                          nullptr, &cnt, nullptr, SVO_MEM_HOST));
        compact2(mask, refPts, trkPts);
    }

    // ---- src/triangulation.cpp:73-166 (both branches of DENSE_FLAG; FAST_FLAG, else GFTT_FLAG: the dense branch's key-point source) ----
    void stereoTriangulate(const Mat &im1, const Mat &im2, std::vector<Point3f> &ref3dPts,
                           std::vector<Point2f> &ref2dPts)
    {
        if (mat_data(im1) == nullptr || mat_data(im2) == nullptr) {
            std::printf("NULL IMG\n");  // src/triangulation.cpp:81-84
            return;
        }
        std::vector<Point2f> refPts, trkPts;
        if (DENSE_FLAG) {
            std::vector<KeyPoint> dkps = FAST_FLAG   ? fastKeypointExtractor(im1)
                                         : GFTT_FLAG ? gfttKeypointExtractor(im1)
                                                     : denseKeypointExtractor(im1, gridStep);
            for (const KeyPoint &k : dkps)
                refPts.emplace_back(k.pt);
            denseLKtracking(im1, im2, refPts, trkPts);
            FmatThresholding(refPts, trkPts);
        } else if (SURF_FLAG) {
            if (mat_cols(im1) != mat_cols(im2) || mat_rows(im1) != mat_rows(im2) || mat_channels(im1) != mat_channels(im2))
                throw SvoError(SVO_ERR_ARG, "stereoTriangulate: the two images differ in size");
            surf_ratio_pairs(ctx_, im1, im2, (double)surfHessian, refPts, trkPts, sparseMatch());
        } else if (STAR_FLAG) {
            starBriefRatioPairs(im1, im2, refPts, trkPts);  // no FmatThresholding, as the ORB branch beside it
        } else {
            orbRatioPairs(im1, im2, refPts, trkPts);  // no FmatThresholding in this branch, as upstream
        }
        // getColors (include/monoUtils.h:180-193)
        svo_pyramid *p = nullptr;
        check(svo_pyramid_create(ctx_, mat_cols(im1), mat_rows(im1), mat_channels(im1), 1, &p));
        colors.assign(refPts.size(), Point3f());
        int rc = svo_pyramid_build(ctx_, p, mat_data(im1), SVO_MEM_HOST);
        if (rc == SVO_OK)
            rc = svo_get_colors(ctx_, p, f(refPts), (int)refPts.size(), f3(colors), SVO_MEM_HOST);
        svo_pyramid_destroy(ctx_, p);
        check(rc);
        double P1[12], P2[12];
        check(svo_stereo_projections(focal_x, focal_y, cx, cy, baseline, P1, P2));
        std::vector<Point3f> xyz(refPts.size());
        check(svo_triangulate(ctx_, P1, P2, f(refPts), f(trkPts), (int)refPts.size(), f3(xyz), nullptr, SVO_MEM_HOST));
        ref3dPts = xyz;
        ref2dPts = refPts;
    }

    // ---- src/tracking.cpp:46-91 (refPts / ref3dpts by value, as upstream) ----
    void PyrLKtrackFrame2Frame(const Mat &refimg, const Mat &curImg, std::vector<Point2f> refPts,
                               std::vector<Point3f> ref3dpts, std::vector<Point2f> &refRetpts,
                               std::vector<Point3f> &ref3dretPts)
    {
        std::vector<Point2f> trackPts(refPts.size());
        std::vector<uint8_t> status(refPts.size());
        lk(refimg, curImg, refPts, trackPts, status);
        std::vector<Point2f> inlierRefPts, inlierTracked, finalInlierRef;
        std::vector<Point3f> inlierRef3dPts;
        for (size_t j = 0; j < refPts.size(); j++)
            if (status[j] == 1) {
                inlierRefPts.push_back(refPts[j]);
                inlierRef3dPts.push_back(ref3dpts[j]);
                inlierTracked.push_back(trackPts[j]);
            }
        std::vector<uint8_t> inIdx(inlierRefPts.size());
        int cnt = 0;
        check(svo_fransac(ctx_, f(inlierRefPts), f(inlierTracked), (int)inlierRefPts.size(), 1.0, 0.99, 1000,
                          ransacSeed + 0, inIdx.data(), nullptr, &cnt, nullptr, SVO_MEM_HOST));
        // the reference loops to refPts.size() here and reads past the compacted arrays
        // (src/tracking.cpp:78); the mask length is what was meant
        for (size_t j = 0; j < inIdx.size(); j++)
            if (inIdx[j] == 1) {
                finalInlierRef.push_back(inlierRefPts[j]);
                ref3dretPts.push_back(inlierRef3dPts[j]);
                refRetpts.push_back(inlierTracked[j]);
            }
        refDrawPts = finalInlierRef;
        trackedDrawPts = refRetpts;
        inlierReferencePyrLKPts = finalInlierRef;
    }

    // ---- dump.cpp:331-348: the measurement of a loop closure, X_ref^-1 X_match, into lcMeasurementT ----
    // PyrLKtrackFrame2Frame(imref, imtrk, refKF.refPts, refKF.pts3d) + solvePnPRansac(100, 0.1, 0.999) + Rodrigues, R = R.t(),
    // tv = -R * tv as ONE library call (svo_closure_measure, seeds ransacSeed + 1 / + 2).  The dump's call site is commented
    // out (:401) and nothing there looks at the inlier count: here fewer than 6 inliers return false and leave lcMeasurementT
    // as it was.  With poseGraph.MEASURED_LC_FLAG set, poseGraph.addLoopClosure(lcMeasurementT, matchKF.idx) uses it.
    struct metaData {
        int idx = 0;
        std::vector<Point2f> refPts;
        std::vector<Point3f> pts3d;  // in the camera frame of frame idx
    };
    Isometry3d lcMeasurementT = Isometry3d::Identity();
    int lcMeasurementTracked = 0, lcMeasurementInliers = 0;
    bool getLCMeasurement(const Mat &imref, const Mat &imtrk, const std::vector<Point2f> &refPts, const std::vector<Point3f> &pts3d)
    {
        if (mat_rows(imref) != mat_rows(imtrk) || mat_cols(imref) != mat_cols(imtrk) || mat_channels(imref) != mat_channels(imtrk) ||
            refPts.size() != pts3d.size())
            throw SvoError(SVO_ERR_ARG, "getLCMeasurement: the images differ in size, or the point sets in length");
        svo_closure_params prm;
        svo_closure_default_params(&prm);
        prm.seed = ransacSeed;
        const double K4[4] = {focal_x, focal_y, cx, cy};
        double z[7];
        const int rc = svo_closure_measure(ctx_, mat_data(imref), mat_data(imtrk), mat_cols(imref), mat_rows(imref),
                                           mat_channels(imref), f(refPts), f3(pts3d), (int)refPts.size(), K4, &prm, z,
                                           &lcMeasurementTracked, &lcMeasurementInliers, SVO_MEM_HOST);
        if (rc == SVO_ERR_TRACKING_LOST)
            return false;
        check(rc);
        lcMeasurementT = pose7_to_iso(z);
        return true;
    }
    bool getLCMeasurement(const metaData &refKF, const metaData &matchKF)
    {
        return getLCMeasurement(loadImageL(refKF.idx), loadImageL(matchKF.idx), refKF.refPts, refKF.pts3d);
    }

    // ---- src/keyFrameManagement.cpp:33-46 ----
    std::vector<Point3f> update3dtransformation(std::vector<Point3f> &pt3d, const Mat34d &pose4dTransform)
    {
        std::vector<Point3f> out(pt3d.size());
        check(svo_transform_points(ctx_, pose4dTransform.m, f3(pt3d), (int)pt3d.size(), f3(out), SVO_MEM_HOST));
        return out;
    }

    // the reference's own signature (include/visualSLAM.h:165): pose4dTransform is a 3x4 CV_64F cv::Mat
    std::vector<Point3f> update3dtransformation(std::vector<Point3f> &pt3d, Mat &pose4dTransform)
    {
        return update3dtransformation(pt3d, mat34_of(pose4dTransform));
    }

    // ---- src/optimizationStuff.cpp:49-64: ORB features + DLoopDetector::detectLoop on the GPU.
    //      One call per frame, in order (the detector stores every frame).  lcParams may be
    //      edited before the first call; result.match / result.query are kept in lastLoopResult. ----
    svo_lc_params lcParams = default_lc_params();
    struct LoopResult {
        int status = SVO_LC_CLOSE_MATCHES_ONLY, query = -1, match = -1;
        bool detection() const { return status == SVO_LC_LOOP_DETECTED; }
    } lastLoopResult;
    void checkLoopDetectorStatus(const Mat &img, int idx)
    {
        if (!lc_)
            check(svo_lc_create(ctx_, &lcParams, mat_cols(img), mat_rows(img), mat_channels(img), &lc_));
        LoopResult r;
        check(svo_lc_detect(lc_, mat_data(img), SVO_MEM_HOST, &r.status, &r.query, &r.match));
        lastLoopResult = r;
        if (r.detection() && (r.query - r.match > loopMinGap) && cooldownTimer == 0) {  // :58
            std::fprintf(stderr, "Found Loop Closure between %d and %d\n", idx, r.match);
            LC_FLAG = true;
            LCidx = r.match - 1;  // :61 (vertices[-1] when match == 0: callers clamp, see processFrame)
            cooldownTimer = loopCooldown;
        }
    }

    // ---- src/rosFuncs.cpp:9-39: far-point filter (-z > 500) + statistical outlier removal
    //      (mean_k 200, stddev multiplier 0.01); colorMap is B,G,R per point and is filtered alike ----
    void SORcloud(std::vector<Point3f> &ref3d, std::vector<Point3f> &colorMap)
    {
        const int n = (int)ref3d.size();
        std::vector<Point3f> p(ref3d.size()), c(colorMap.size());
        int kept = 0;
        const bool with_color = colorMap.size() == ref3d.size() && n > 0;
        check(svo_sor_filter(ctx_, f3(ref3d), with_color ? f3(colorMap) : nullptr, n, 200, 0.01, 500.f, f3(p),
                             with_color ? f3(c) : nullptr, &kept, nullptr, nullptr, SVO_MEM_HOST));
        p.resize((size_t)kept);
        ref3d = p;
        if (with_color) {
            c.resize((size_t)kept);
            colorMap = c;
        } else
            colorMap.clear();
    }

    // ---- src/keyFrameManagement.cpp:9-31 ----
    void insertKeyFrames(int /*start*/, const Mat &imL, const Mat &imR, const Mat34d &pose4dTransform,
                         std::vector<Point2f> &ftrPts, std::vector<Point3f> &ref3dCoords)
    {
        std::vector<Point2f> new2d;
        std::vector<Point3f> new3d;
        ftrPts.clear();
        ref3dCoords.clear();
        stereoTriangulate(imL, imR, new3d, new2d);
        untransformed = new3d;
        ref3dCoords = update3dtransformation(new3d, pose4dTransform);
        ftrPts = new2d;
    }

    // the reference's own signature (include/visualSLAM.h:164): images by value, pose4dTransform a 3x4
    // CV_64F cv::Mat
    void insertKeyFrames(int start, Mat imL, Mat imR, Mat &pose4dTransform, std::vector<Point2f> &ftrPts,
                         std::vector<Point3f> &ref3dCoords)
    {
        insertKeyFrames(start, imL, imR, mat34_of(pose4dTransform), ftrPts, ref3dCoords);
    }

    // ---- src/keyFrameManagement.cpp:73-94 (uses the members referenceImg / currentImage) ----
    void PerspectiveNpointEstimation(Mat & /*prevImg*/, Mat & /*curImg*/, std::vector<Point2f> &ref2dPoints,
                                     std::vector<Point3f> &ref3dPoints, std::vector<Point2f> &tracked2dPoints,
                                     std::vector<Point3f> &tracked3dPoints, Vec3d &rvec, Vec3d &tvec,
                                     std::vector<int> &inliers)
    {
        PyrLKtrackFrame2Frame(referenceImg, currentImage, ref2dPoints, ref3dPoints, tracked2dPoints, tracked3dPoints);
        const double K4[4] = {focal_x, focal_y, cx, cy};
        const int n = (int)tracked3dPoints.size();
        int ninl = 0;
        inliers.assign((size_t)(n > 0 ? n : 1), 0);
        check(svo_pnp_ransac(ctx_, f3(tracked3dPoints), f(tracked2dPoints), n, K4, 100, 1.0, 0.99, ransacSeed + 1,
                             rvec.v, tvec.v, inliers.data(), &ninl, nullptr, SVO_MEM_HOST));
        if (ninl < 10) {
            std::printf("Low inlier count at %d, trying again with increased reprojection Threshold \n", ninl);
            check(svo_pnp_ransac(ctx_, f3(tracked3dPoints), f(tracked2dPoints), n, K4, 100, 8.0, 0.98, ransacSeed + 2,
                                 rvec.v, tvec.v, inliers.data(), &ninl, nullptr, SVO_MEM_HOST));
            if (ninl < 10)
                SHUTDOWN_FLAG = true;  // src/keyFrameManagement.cpp:89-92
        }
        inliers.resize((size_t)ninl);
    }

    // the reference's own signature (include/visualSLAM.h:168-169): rvec / tvec come back as 3x1 CV_64F
    // cv::Mat, as cv::solvePnPRansac fills them
    void PerspectiveNpointEstimation(Mat &prevImg, Mat &curImg, std::vector<Point2f> &ref2dPoints,
                                     std::vector<Point3f> &ref3dPoints, std::vector<Point2f> &tracked2dPoints,
                                     std::vector<Point3f> &tracked3dPoints, Mat &rvec, Mat &tvec,
                                     std::vector<int> &inliers)
    {
        Vec3d r, t;
        PerspectiveNpointEstimation(prevImg, curImg, ref2dPoints, ref3dPoints, tracked2dPoints, tracked3dPoints, r, t,
                                    inliers);
        rvec = to_mat(r);
        tvec = to_mat(t);
    }

    // ---- src/optimizationStuff.cpp:3-15 ----
    // the reference's own signature (include/visualSLAM.h:177): four CV_64F cv::Mat (R 3x3; t 3x1 --
    // cvMat2Eigen reads tvec.at<double>(i, 0), include/monoUtils.h:102-104; a 1x3 t is accepted too)
    void stageForPGO(Mat Rl, Mat tl, Mat Rg, Mat tg, bool loopClose)
    {
        stageForPGO(mat33_of(Rl), vec3_of(tl), mat33_of(Rg), vec3_of(tg), loopClose);
    }
    void stageForPGO(const Mat33d & /*Rl*/, const Vec3d & /*tl*/, const Mat33d &Rg, const Vec3d &tg, bool loopClose)
    {
        const Isometry3d globalT = Isometry3d_from(Rg, tg);
        if (loopClose) {
            LC_FLAG = true;
            poseGraph.addLoopClosure(globalT, LCidx);
        } else {
            poseGraph.augmentNode(globalT, globalT);
        }
    }

    // ---- src/optimizationStuff.cpp:17-47 ----
    // trajectory <- translations of T; every stored record's camera-frame cloud re-transformed with
    // [R_old | t_new]; mapHistory rebuilt from the records with retrack.  Records that processFrame
    // stored keep their clouds in HBM (svo_map): ONE launch re-transforms all of them.  Records a
    // caller pushed into keyFrameHistory with a host cloud go through update3dtransformation as upstream.
    void updateOdometry(std::vector<Isometry3d> &T)
    {
        trajectory.clear();
        trajectory.reserve(T.size());
        for (const Isometry3d &iso : T)
            trajectory.push_back(translation_of(iso));
        mapHistory.clear();
        if (map_ && svo_map_num_keyframes(map_) > 0) {
            std::vector<double> ts(trajectory.size() * 3);
            for (size_t j = 0; j < trajectory.size(); j++)
                for (int i = 0; i < 3; i++)
                    ts[3 * j + i] = trajectory[j](i);
            check(svo_map_update(map_, ts.data(), (int)trajectory.size()));
            for (size_t j = 0; j < keyFrameHistory.size() && j < trajectory.size(); j++)
                keyFrameHistory[j].t = trajectory[j];  // R keeps its un-optimised value, as upstream (:29-32)
            size_t npts = 0;
            int nkf = 0;
            check(svo_map_get_points(map_, nullptr, 0, nullptr, 0, &npts, &nkf, SVO_MEM_HOST));
            std::vector<Point3f> all(npts);
            std::vector<int> counts((size_t)nkf);
            check(svo_map_get_points(map_, f3(all), npts, counts.data(), nkf, &npts, &nkf, SVO_MEM_HOST));
            size_t o = 0;
            for (int k = 0; k < nkf; k++) {
                mapHistory.emplace_back(all.begin() + (long)o, all.begin() + (long)(o + (size_t)counts[k]));
                o += (size_t)counts[k];
            }
            return;
        }
        for (size_t j = 0; j < keyFrameHistory.size() && j < trajectory.size(); j++) {
            keyFrame &kf = keyFrameHistory[j];
            kf.t = trajectory[j];  // R keeps its un-optimised value, as upstream (:29-32)
            Mat34d P = Mat34d::from(kf.R, kf.t);
            std::vector<Point3f> upd = update3dtransformation(kf.ref3dCoords, P);
            if (kf.retrack)
                mapHistory.emplace_back(upd);
        }
    }

    // ---- the loop body of initSequence (src/VisualSLAM.cpp:54-169) on the fused front-end ----
    // First call = frame 0 (stereo init, src/VisualSLAM.cpp:22-41).  loopMatch >= 0 plays the role
    // of DLoopDetector's result.match for this frame (src/optimizationStuff.cpp:59-63).
    // Returns false when tracking is lost (SHUTDOWN_FLAG).
    bool processFrame(const Mat &left, const Mat &right, int loopMatch, Mat33d &R, Vec3d &t)
    {
        if (!vo_) {
            svo_vo_params p;
            svo_vo_default_params(&p);
            p.fx = focal_x;
            p.fy = focal_y;
            p.cx = cx;
            p.cy = cy;
            p.baseline = baseline;
            p.grid_step = gridStep;
            p.keyframe_min_inliers = keyframeMinInliers;
            p.seed = ransacSeed;
            check(svo_vo_create(ctx_, &p, mat_cols(left), mat_rows(left), mat_channels(left), &vo_));
            int n = 0;
            check(svo_vo_init(vo_, mat_data(left), mat_data(right), SVO_MEM_HOST, &n));
            poseGraph.initializeGraph();
            R = Mat33d();
            t = Vec3d();
            keyFrame kf;  // src/VisualSLAM.cpp:35-37: kf.ref3dCoords = ref3dCoords, retrack stays false
            kf.idx = 0;
            store_record(kf, R, t, false, 0);
            keyFrameHistory.push_back(kf);
            isoVector.push_back(Isometry3d_from(R, t));
            frame_ = 0;
            return true;
        }
        frame_++;
        int ninl = 0, ntrk = 0;
        int rc = svo_vo_localize(vo_, mat_data(left), SVO_MEM_HOST, R.m, t.v, &ninl, &ntrk);
        if (rc == SVO_ERR_TRACKING_LOST) {
            SHUTDOWN_FLAG = true;
            return false;
        }
        check(rc);
        // checkLoopDetectorStatus (src/optimizationStuff.cpp:59-63) with the supplied match
        if (loopMatch >= 0 && (frame_ - loopMatch > loopMinGap) && cooldownTimer == 0) {
            LC_FLAG = true;
            LCidx = loopMatch > 0 ? loopMatch - 1 : 0;  // the reference indexes vertices[-1] when match == 0
            cooldownTimer = loopCooldown;
        }
        if (LC_FLAG) {  // src/VisualSLAM.cpp:76-86
            stageForPGO(R, t, R, t, true);
            stageForPGO(R, t, R, t, false);
            std::vector<Isometry3d> trans = poseGraph.globalOptimize();
            isoVector = trans;
            t = translation_of(trans.back());  // only t is re-anchored, R keeps its value (:81-82)
            updateOdometry(trans);
        } else {
            stageForPGO(R, t, R, t, false);
        }
        int kf = 0;
        check(svo_vo_update(vo_, mat_data(right), SVO_MEM_HOST, R.m, t.v, ninl, LC_FLAG ? 1 : 0, &kf));
        if (kf) {  // src/VisualSLAM.cpp:122-140
            // good3d = the new reference cloud (world) with its colours -- stereoTriangulate's `colors` member, gathered
            // by the fused path's triangulation launch --, SORcloud'ed together, appended to mapHistory / colorHistory
            // (src/VisualSLAM.cpp:125-136)
            const int cap = svo_vo_capacity(vo_);
            std::vector<Point3f> good3d((size_t)cap), goodColors((size_t)cap);
            int n = 0, nc = 0;
            check(svo_vo_get_reference(vo_, nullptr, f3(good3d), cap, &n, SVO_MEM_HOST));
            check(svo_vo_get_keyframe_colors(vo_, f3(goodColors), cap, &nc, SVO_MEM_HOST));
            good3d.resize((size_t)n);
            goodColors.resize((size_t)(nc == n ? n : 0));  // point for point with the cloud, or none
            colors = goodColors;
            if (mapSOR && n > 0)
                SORcloud(good3d, goodColors);
            mapHistory.emplace_back(good3d);
            colorHistory.emplace_back(goodColors);
            isoVector.push_back(Isometry3d_from(R, t));
            trajectory.push_back(t);
        }
        if (cooldownTimer != 0)
            cooldownTimer--;
        LC_FLAG = false;
        keyFrame k;  // src/VisualSLAM.cpp:154-166
        k.idx = frame_;
        k.R = R;
        k.t = t;
        k.retrack = kf != 0;
        if (kf)
            store_record(k, R, t, true, frame_);
        keyFrameHistory.push_back(k);
        return true;
    }

  private:
    static const float *f(const std::vector<Point2f> &v) { return reinterpret_cast<const float *>(v.data()); }
    static float *f(std::vector<Point2f> &v) { return reinterpret_cast<float *>(v.data()); }
    static const float *f3(const std::vector<Point3f> &v) { return reinterpret_cast<const float *>(v.data()); }
    static float *f3(std::vector<Point3f> &v) { return reinterpret_cast<float *>(v.data()); }
    static Isometry3d Isometry3d_from(const Mat33d &R, const Vec3d &t) { return iso_from(R, t); }
    static Vec3d translation_of(const Isometry3d &T)
    {
        Vec3d t;
        for (int i = 0; i < 3; i++)
            t(i) = T(i, 3);
        return t;
    }
    void lk(const Mat &a, const Mat &b, const std::vector<Point2f> &pts, std::vector<Point2f> &out,
            std::vector<uint8_t> &status)
    {
        svo_pyramid *pa = nullptr, *pb = nullptr;
        check(svo_pyramid_create(ctx_, mat_cols(a), mat_rows(a), mat_channels(a), 4, &pa));
        int rc = svo_pyramid_create(ctx_, mat_cols(b), mat_rows(b), mat_channels(b), 4, &pb);
        if (rc == SVO_OK)
            rc = svo_pyramid_build(ctx_, pa, mat_data(a), SVO_MEM_HOST);
        if (rc == SVO_OK)
            rc = svo_pyramid_build(ctx_, pb, mat_data(b), SVO_MEM_HOST);
        if (rc == SVO_OK)
            rc = svo_lk_track(ctx_, pa, pb, f(pts), (int)pts.size(), f(out), status.data(), nullptr, nullptr,
                              SVO_MEM_HOST);
        svo_pyramid_destroy(ctx_, pa);
        svo_pyramid_destroy(ctx_, pb);
        check(rc);
    }
    // src/triangulation.cpp:105-133: ORB::create(orbFeatures) on both images (one set of launches), desc.convertTo(CV_32F) +
    // BFMatcher().knnMatch(desc1, desc2, matches, 2) = the L2 norm of the descriptor bytes, m.distance < 0.8 * n.distance
    void orbRatioPairs(const Mat &im1, const Mat &im2, std::vector<Point2f> &pt1, std::vector<Point2f> &pt2)
    {
        if (mat_cols(im1) != mat_cols(im2) || mat_rows(im1) != mat_rows(im2) || mat_channels(im1) != mat_channels(im2))
            throw SvoError(SVO_ERR_ARG, "stereoTriangulate: the two images differ in size");
        svo_orb_params prm;
        svo_orb_default_params(&prm);
        prm.n_features = orbFeatures;
        const size_t nf = (size_t)(orbFeatures > 0 ? orbFeatures : 0);
        const uint8_t *imgs[2] = {mat_data(im1), mat_data(im2)};
        std::vector<Point2f> kp(2 * nf);
        std::vector<uint32_t> desc(2 * nf * 8);
        int n[2] = {0, 0};
        check(svo_orb_extract_batch(ctx_, imgs, 2, mat_cols(im1), mat_rows(im1), mat_channels(im1), &prm, f(kp), nullptr, nullptr,
                                    nullptr, desc.data(), n, SVO_MEM_HOST));
        sparse_match_points(ctx_, sparseMatch(), SVO_MATCH_L2_U8, desc.data(), desc.data() + nf * 8, 32, n[0], n[1], f(kp), f(kp) + 2 * nf, pt1,
                            pt2);
    }
    // n (1 ... 16) images of one size through one svo_star_detect_batch call.  The capacity grows to what the library asks for, so a
    // call never loses key points.
    void starKeypointsBatch(const Mat *const *imgs, int n, std::vector<KeyPoint> *kps)
    {
        const uint8_t *ptrs[16];
        same_size_ptrs(imgs, n, "starKeypointExtractor", ptrs);
        const Mat &first = *imgs[0];
        svo_star_params prm;
        svo_star_default_params(&prm);
        prm.max_size = starMaxSize;
        prm.response_threshold = starResponseThreshold;
        size_t cap = 4096;
        std::vector<float> xy, size, resp;
        std::vector<int> cnt((size_t)n);
        for (;;) {
            const size_t e = cap * (size_t)n;
            xy.resize(2 * e);
            size.resize(e);
            resp.resize(e);
            const int rc = svo_star_detect_batch(ctx_, ptrs, n, mat_cols(first), mat_rows(first), mat_channels(first), &prm, (int)cap,
                                                 xy.data(), size.data(), resp.data(), cnt.data(), SVO_MEM_HOST);
            size_t need = 0;
            for (int i = 0; i < n; i++)
                need = (size_t)cnt[(size_t)i] > need ? (size_t)cnt[(size_t)i] : need;
            if (rc == SVO_ERR_CAPACITY && need > cap) {
                cap = need;  // every count is the needed one
                continue;
            }
            check(rc);
            break;
        }
        for (int i = 0; i < n; i++) {
            const size_t b = cap * (size_t)i, m = (size_t)cnt[(size_t)i];
            kps[i].clear();
            kps[i].reserve(m);
            for (size_t j = 0; j < m; j++) {
                kps[i].emplace_back(xy[2 * (b + j)], xy[2 * (b + j) + 1], size[b + j]);
                kps[i].back().angle = -1.f;
                kps[i].back().response = resp[b + j];
                kps[i].back().octave = 0;
            }
        }
    }
    // src/triangulation.cpp:79-80 in the place of :105-133: Star on both images (one set of launches), brief->compute on both (one
    // svo_brief_describe_batch call, 32 bytes; the key points runByImageBorder(28) removes are dropped, as cv erases them),
    // desc.convertTo(CV_32F) + BFMatcher().knnMatch(desc1, desc2, matches, 2), m.distance < 0.8 * n.distance
    void starBriefRatioPairs(const Mat &im1, const Mat &im2, std::vector<Point2f> &pt1, std::vector<Point2f> &pt2)
    {
        const Mat *imgs[2] = {&im1, &im2};
        const uint8_t *ptrs[2];
        same_size_ptrs(imgs, 2, "stereoTriangulate", ptrs);
        std::vector<KeyPoint> kps[2];
        starKeypointsBatch(imgs, 2, kps);
        const size_t cap = std::max<size_t>(std::max(kps[0].size(), kps[1].size()), 1);
        std::vector<float> xy(2 * 2 * cap, 0.f);
        int n_in[2], n_out[2] = {0, 0};
        for (int i = 0; i < 2; i++) {
            n_in[i] = (int)kps[i].size();
            for (size_t j = 0; j < kps[i].size(); j++) {
                xy[2 * (cap * (size_t)i + j)] = kps[i][j].pt.x;
                xy[2 * (cap * (size_t)i + j) + 1] = kps[i][j].pt.y;
            }
        }
        std::vector<int> kept(2 * cap);
        std::vector<uint8_t> desc(2 * cap * 32);
        check(svo_brief_describe_batch(ctx_, ptrs, 2, mat_cols(im1), mat_rows(im1), mat_channels(im1), 32, xy.data(), n_in, (int)cap,
                                       kept.data(), desc.data(), n_out, SVO_MEM_HOST));
        std::vector<float> kxy(2 * 2 * cap, 0.f);
        for (int i = 0; i < 2; i++)
            for (int j = 0; j < n_out[i]; j++) {
                const size_t src = cap * (size_t)i + (size_t)kept[cap * (size_t)i + (size_t)j], dst = cap * (size_t)i + (size_t)j;
                kxy[2 * dst] = xy[2 * src];
                kxy[2 * dst + 1] = xy[2 * src + 1];
            }
        sparse_match_points(ctx_, sparseMatch(), SVO_MATCH_L2_U8, desc.data(), desc.data() + cap * 32, 32, n_out[0], n_out[1], kxy.data(),
                            kxy.data() + 2 * cap, pt1, pt2);
    }
    void compact2(const std::vector<uint8_t> &mask, std::vector<Point2f> &a, std::vector<Point2f> &b)
    {
        std::vector<Point2f> oa(a.size()), ob(b.size());
        int cnt = 0;
        check(svo_compact(ctx_, mask.data(), (int)mask.size(), f(a), 2, f(oa), f(b), 2, f(ob), nullptr, 0, nullptr, &cnt,
                          SVO_MEM_HOST));
        oa.resize((size_t)cnt);
        ob.resize((size_t)cnt);
        a.swap(oa);
        b.swap(ob);
    }

    // The fused front-end's last keyframe cloud (camera frame, `untransformed`) becomes the record's
    // cloud: SORcloud first when mapSOR (src/VisualSLAM.cpp:154), then into the device map.  Upstream
    // stores the same cloud again in every non-keyframe record and re-transforms it on every closure only
    // to discard the result (src/optimizationStuff.cpp:43-45); those copies are not kept here.
    void store_record(keyFrame &k, const Mat33d &R, const Vec3d &t, bool retrack, int traj_index)
    {
        if (!map_)
            check(svo_map_create(ctx_, &map_));
        int n = 0;
        check(svo_vo_get_keyframe_cloud(vo_, nullptr, 0, &n, SVO_MEM_HOST));
        std::vector<Point3f> cloud((size_t)n);
        if (n > 0)
            check(svo_vo_get_keyframe_cloud(vo_, f3(cloud), n, &n, SVO_MEM_HOST));
        untransformed = cloud;
        if (mapSOR && n > 0) {
            std::vector<Point3f> none;
            SORcloud(untransformed, none);
        }
        k.ref3dCoords = untransformed;
        check(svo_map_add_keyframe(map_, traj_index, R.m, t.v, f3(untransformed), (int)untransformed.size(),
                                   retrack ? 1 : 0, SVO_MEM_HOST));
    }

    svo_ctx *ctx_;
    svo_vo *vo_ = nullptr;
    svo_lc *lc_ = nullptr;
    svo_map *map_ = nullptr;
    static Mat load_frame(const char *pattern, int iter)
    {
        char path[1024];
        int w = 0, h = 0, c = 0;
        if (!pattern || svo_io_format_path(path, (int)sizeof(path), pattern, iter) != SVO_OK ||
            svo_io_image_info(path, &w, &h, &c) != SVO_OK) {
            std::fprintf(stderr, "yikes, failed to fetch frame, check the paths\n");
            return Mat();
        }
        Mat im(h, w, CV_8UC3);
        uint8_t *dst = im.data;
        if (svo_io_read_image(path, 3, dst, (size_t)w * h * 3, &w, &h) != SVO_OK) {
            std::fprintf(stderr, "yikes, failed to fetch frame, check the paths\n");
            return Mat();
        }
        return im;
    }
    static svo_lc_params default_lc_params()
    {
        svo_lc_params p;
        svo_lc_default_params(&p);
        return p;
    }
    int frame_ = 0;
};

}  // namespace svo_compat
