"""``KeyframeWindow``: the observations a keyframe's lattice points collect until the next keyframe is cut, and their joint
adjustment by ``svo_ba_window``.  A keyframe's points are seen in its stereo pair and, through LK, in every
frame tracked from it; the window records those observations with the PnP pose of each frame, builds the CSR arrays and lets the
library refine poses and points together, the keyframe's pose held.

Plumbing only: grid sampling, LK, the F-matrix filters, triangulation, the compactions, PnP-RANSAC and the adjustment are library
calls; the host builds index arrays.  The fused ``svo_vo_*`` runner is a different path and is not touched by this module.
"""
from __future__ import annotations

import numpy as np

from . import capi
from .prototype import rodrigues

GRID_STEP = 30            # src/triangulation.cpp:89
F_THR_STEREO = 3.0        # src/tracking.cpp:34
F_THR_TEMPORAL = 1.0      # src/tracking.cpp:75
PNP_ITERATIONS, PNP_REPROJ, PNP_CONFIDENCE = 100, 1.0, 0.99


def _image(im) -> np.ndarray:
    im = np.ascontiguousarray(im, np.uint8)
    return im.reshape(im.shape[0], im.shape[1], -1)


class KeyframeWindow:
    """``KeyframeWindow(ctx, K4, baseline, seed)``: K4 = (fx, fy, cx, cy).  ``open`` starts a window at a stereo pair, ``add``
    tracks one more left image, ``adjust`` runs the bundle adjustment.  Poses are world -> camera with the keyframe as the world."""

    def __init__(self, ctx: capi.Context, K4, baseline: float, seed: int = 0, grid_step: int = GRID_STEP):
        self.ctx, self.K4, self.baseline, self.seed = ctx, tuple(float(v) for v in K4), float(baseline), int(seed)
        self.grid_step = int(grid_step)
        self.P1, self.P2 = capi.stereo_projections(*self.K4, self.baseline)
        self._pyr = None
        self.points3d = np.zeros((0, 3), np.float32)   # the keyframe's points, camera frame of the keyframe
        self.poses = []                                # R9 | t3 per frame, the keyframe (identity) first
        self.observations = []                         # per frame: (point ids int32 [m], uvr float32 [m, 3])

    def _pyramids(self, shape):
        h, w, c = shape
        if self._pyr is None or self._pyr[0] != (w, h, c):
            self._pyr = ((w, h, c), [self.ctx.pyramid(w, h, c) for _ in range(3)])
        return self._pyr[1]

    @staticmethod
    def _ids(column) -> np.ndarray:
        return np.ascontiguousarray(column).view(np.int32).reshape(-1)

    def open(self, left, right) -> int:
        """Grid -> stereo LK -> status compaction -> stereo F filter -> triangulation; every kept point's stereo observation in the
        keyframe is recorded.  -> the number of points."""
        l, r = _image(left), _image(right)
        a, b, _ = self._pyramids(l.shape)
        a.build(l)
        b.build(r)
        grid = self.ctx.grid_keypoints(l.shape[0], l.shape[1], self.grid_step)
        trk, status, _, _ = self.ctx.lk_track(a, b, grid)
        pl, pr = self.ctx.compact(status, grid, trk)
        _, mask, _, _ = self.ctx.fransac(pl, pr, F_THR_STEREO, 0.99, 1000, self.seed)
        pl, pr = self.ctx.compact(mask, pl, pr)
        xyz, _ = self.ctx.triangulate(self.P1, self.P2, pl, pr)
        n = len(pl)
        self.points3d = xyz
        self.poses = [np.r_[np.eye(3).ravel(), np.zeros(3)]]
        self.observations = [(np.arange(n, dtype=np.int32), np.ascontiguousarray(np.c_[pl, pr[:, 0]], dtype=np.float32))]
        self._prev_pts, self._prev_ids, self._frame = pl, np.arange(n, dtype=np.int32), 1
        self._cur = 0   # which of the two left pyramids holds the previous frame
        return n

    def add(self, left) -> int:
        """LK from the previous frame, the status compaction (the int32 point-id column rides through ``ctx.compact`` beside the
        points), the temporal F filter, PnP-RANSAC against the keyframe's points; the inliers' observations and the PnP pose are
        recorded.  -> the number of inliers."""
        img = _image(left)
        pyrs = self._pyramids(img.shape)
        prev, cur = pyrs[0 if self._cur == 0 else 2], pyrs[2 if self._cur == 0 else 0]
        cur.build(img)
        trk, status, _, _ = self.ctx.lk_track(prev, cur, self._prev_pts)
        ids_f = self._prev_ids.view(np.float32).reshape(-1, 1)   # the bits of the ids, moved as one float column
        p0, p1, idc = self.ctx.compact(status, self._prev_pts, trk, ids_f)
        _, mask, _, _ = self.ctx.fransac(p0, p1, F_THR_TEMPORAL, 0.99, 1000, self.seed + self._frame)
        _, p1, idc = self.ctx.compact(mask, p0, p1, idc)
        ids = self._ids(idc)
        cnt, rvec, tvec, inl, _ = self.ctx.pnp_ransac(self.points3d[ids], p1, self.K4, PNP_ITERATIONS, PNP_REPROJ, PNP_CONFIDENCE,
                                                      self.seed + self._frame)
        self.poses.append(np.r_[rodrigues(rvec).ravel(), np.asarray(tvec, np.float64).reshape(3)])
        uvr = np.full((cnt, 3), np.nan, np.float32)
        uvr[:, :2] = p1[inl]
        self.observations.append((np.ascontiguousarray(ids[inl]), uvr))
        self._prev_pts, self._prev_ids = np.ascontiguousarray(p1), np.ascontiguousarray(ids)
        self._cur = 2 if self._cur == 0 else 0
        self._frame += 1
        return cnt

    def arrays(self):
        """The arguments of ``ctx.ba_window``: (poses, fixed, pts3d, obs_start, obs_pose, obs_uvr), CSR by point, a point's
        observations in frame order."""
        n = len(self.points3d)
        ids = np.concatenate([o[0] for o in self.observations])
        pose = np.concatenate([np.full(len(o[0]), j, np.int32) for j, o in enumerate(self.observations)])
        uvr = np.concatenate([o[1] for o in self.observations])
        order = np.argsort(ids, kind="stable")
        start = np.zeros(n + 1, np.int32)
        start[1:] = np.cumsum(np.bincount(ids, minlength=n))
        fixed = np.zeros(len(self.poses), np.uint8)
        fixed[0] = 1
        return (np.array(self.poses), fixed, self.points3d, start, np.ascontiguousarray(pose[order]),
                np.ascontiguousarray(uvr[order]))

    def adjust(self, params=None):
        """-> (poses, points, per-observation chi2, info) of ``ctx.ba_window`` with the keyframe's pose held."""
        if params is None:
            params = {}
        if isinstance(params, dict):
            fx, fy, cx, cy = self.K4
            params = capi.ba_window_params.default(**{**dict(fx=fx, fy=fy, cx=cx, cy=cy, bf=fx * self.baseline), **params})
        return self.ctx.ba_window(*self.arrays(), params=params)
