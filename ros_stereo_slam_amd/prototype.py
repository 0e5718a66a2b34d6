"""The Python prototype's own odometry, ``VisOdometry`` of src/ROSslam.py:144-273, assembled from ``svo_*`` calls (DESIGN.md
section 10k).  It is a different odometry from the keyframe one: the tracked 2-D / 3-D set is topped up on EVERY frame with freshly
triangulated points that duplicate none of the tracked ones, and is never rebuilt at a keyframe.

The method names are the prototype's.  Plumbing only: every piece of arithmetic is a library call (SIFT, exact kNN + ratio test,
triangulation, LK 21 x 21 / 4 levels / 30 / 0.01, PnP-RANSAC with OpenCV's defaults, ``svo_replenish``); there is no CPU fall-back.
Left outside: ROS publishing and the canvas, the ground-truth plot, the display cloud's remove_statistical_outlier (it never feeds
a pose), and FLANN's randomised KD-trees, for which the exact kNN stands in.
"""
from __future__ import annotations

import numpy as np

from . import capi

SIFT_FEATURES = 2000      # cv2.xfeatures2d.SIFT_create(2000), src/ROSslam.py:172
RATIO = 0.8               # m.distance < 0.8 * n.distance, :188
DUP_RADIUS = 5            # removeDuplicate(queryPoints, refPoints, radius=5), :156
PNP_ITERATIONS, PNP_REPROJ, PNP_CONFIDENCE = 100, 8.0, 0.99     # solvePnPRansac(obj, img, K, None): OpenCV's defaults, :247


def rodrigues(rvec) -> np.ndarray:
    """cv2.Rodrigues(rvec)[0]: the rotation matrix of an axis-angle vector."""
    r = np.asarray(rvec, np.float64).reshape(3)
    theta = float(np.linalg.norm(r))
    if theta < np.finfo(np.float64).eps:
        return np.eye(3)
    k = r / theta
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    c, s = np.cos(theta), np.sin(theta)
    return c * np.eye(3) + (1 - c) * np.outer(k, k) + s * Kx


def _image(im) -> np.ndarray:
    im = np.ascontiguousarray(im, np.uint8)
    return im.reshape(im.shape[0], im.shape[1], -1)


class VisOdometry:
    """``VisOdometry(ctx, K4, baseline)``: K4 = (fx, fy, cx, cy).  State, as the prototype names it: ``referenceImage``,
    ``referencePoints2D`` [n, 2] and ``referencePoints3D`` [n, 3] (float32; the prototype keeps float64 points)."""

    def __init__(self, ctx: capi.Context, K4, baseline: float, seed: int = 0, replenish: bool = True):
        self.ctx, self.K4, self.baseline, self.seed = ctx, tuple(float(v) for v in K4), float(baseline), int(seed)
        self.replenishing = bool(replenish)      # False: the same loop with n_new = 0 (what the top-up is measured against)
        self.P1, self.P2 = capi.stereo_projections(*self.K4, self.baseline)
        self.referenceImage = None
        self.referencePoints2D = np.zeros((0, 2), np.float32)
        self.referencePoints3D = np.zeros((0, 3), np.float32)
        self.path = []
        self._pyr = None

    # ---- src/ROSslam.py:171-209 ----
    def matchedPairs(self, lImg, rImg):
        """SIFT(2000) on both images, knnMatch(k = 2), the 0.8 ratio test -> (pts1, pts2) of the surviving pairs."""
        l, r = _image(lImg), _image(rImg)
        (xl, _, _, _, _, dl), (xr, _, _, _, _, dr) = self.ctx.sift_extract([l, r], dict(n_features=SIFT_FEATURES))
        if len(xl) < 1 or len(xr) < 2:
            return np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32)
        idx, dist = self.ctx.knn_match(dl, dr, k=2, norm=capi.MATCH_L2_F32)
        p1, p2, _ = self.ctx.ratio_pairs(idx, dist, xl, xr, RATIO)
        return p1, p2

    def sparseStereoTriangulate(self, lImg, rImg, refPts=None):
        """-> (pts3D [m, 3], pts1 [m, 2]); with refPts the pairs whose left point duplicates one of them go first (BOX, radius 5)."""
        p1, p2 = self.matchedPairs(lImg, rImg)
        if refPts is not None and len(p1):
            mask = self.removeDuplicate(p1, refPts).astype(bool)
            p1, p2 = np.ascontiguousarray(p1[mask]), np.ascontiguousarray(p2[mask])
        if not len(p1):
            return np.zeros((0, 3), np.float32), p1
        xyz, _ = self.ctx.triangulate(self.P1, self.P2, p1, p2)
        return xyz, p1

    # ---- :156-169 ----
    def removeDuplicate(self, queryPoints, refPoints, radius=DUP_RADIUS):
        """The boolean mask of the query points to keep.  Unlike the prototype it leaves queryPoints as they are."""
        return self.ctx.dedup_points(refPoints, queryPoints, radius, capi.DEDUP_BOX).astype(bool)

    # ---- :144-154 ----
    def trackPointsFrame2Frame(self, RefIm, CurIm, refPts, ref3dPts):
        """LK from RefIm to CurIm, then the status compaction -> (pts3dInliers, refInliers, trackInliers)."""
        ref, cur = _image(RefIm), _image(CurIm)
        h, w, c = ref.shape
        if self._pyr is None or self._pyr[0] != (w, h, c):
            self._pyr = ((w, h, c), self.ctx.pyramid(w, h, c), self.ctx.pyramid(w, h, c))
        _, a, b = self._pyr
        a.build(ref)
        b.build(cur)
        refPts = np.ascontiguousarray(refPts, np.float32).reshape(-1, 2)
        ref3dPts = np.ascontiguousarray(ref3dPts, np.float32).reshape(-1, 3)
        if not len(refPts):
            return ref3dPts, refPts, refPts.copy()
        trk, status, _, _ = self.ctx.lk_track(a, b, refPts)
        p3, p2, t2 = self.ctx.compact(status, ref3dPts, refPts, trk)
        return p3, p2, t2

    # ---- :216-227 ----
    def initializeSequence(self, lImg, rImg):
        pts3d, lpts = self.sparseStereoTriangulate(lImg, rImg)
        self.referenceImage = lImg
        self.referencePoints2D, self.referencePoints3D = lpts, pts3d
        return len(lpts)

    # ---- the loop body, :242-273 ----
    def step(self, curIm, curImR):
        """One frame -> (R [3, 3], t [3], n_out, n_dup, n_behind): the pose as the prototype forms it (R = Rodrigues(rvec) transposed,
        t = -R^T tvec) and the counts of the top-up."""
        p3, _, trk = self.trackPointsFrame2Frame(self.referenceImage, curIm, self.referencePoints2D, self.referencePoints3D)
        cnt, rvec, tvec, inl, _ = self.ctx.pnp_ransac(p3, trk, self.K4, PNP_ITERATIONS, PNP_REPROJ, PNP_CONFIDENCE, self.seed)
        self.referencePoints2D, self.referencePoints3D = np.ascontiguousarray(trk[inl]), np.ascontiguousarray(p3[inl])
        R = rodrigues(rvec)
        t = -R.T @ tvec
        inv_transform = np.hstack((R.T, t.reshape(3, 1)))
        # The prototype filters inside sparseStereoTriangulate and moves and appends afterwards; svo_replenish does the filter, the move,
        # the z > 0 test and the append in one call, so the pairs are triangulated unfiltered here (triangulation is per point).
        if self.replenishing:
            new3d, new2d = self.sparseStereoTriangulate(curIm, curImR)
        else:
            new3d, new2d = np.zeros((0, 3), np.float32), np.zeros((0, 2), np.float32)
        self.referencePoints2D, self.referencePoints3D, n_dup, n_behind = self.ctx.replenish(
            self.referencePoints2D, self.referencePoints3D, new2d, new3d, DUP_RADIUS, inv_transform, capi.DEDUP_BOX)
        self.referenceImage = curIm
        self.path.append((R.T.copy(), t.copy()))
        return R.T, t, len(self.referencePoints2D), n_dup, n_behind

    # ---- :229-273 ----
    def trackSequence(self, frames):
        """frames: an iterable of (left, right) images; the first pair initialises.  -> the list of what ``step`` returned."""
        out = []
        for k, (left, right) in enumerate(frames):
            if k == 0:
                self.initializeSequence(left, right)
            else:
                out.append(self.step(left, right))
        return out
