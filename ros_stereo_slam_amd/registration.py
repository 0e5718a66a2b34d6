"""PoseGraphOptimize of the Python prototype (src/ROSslam.py:34-73) on the library's own ICP: pairwiseRegistration is a
coarse and a fine point-to-plane registration and the information matrix at the fine distance (``svo_icp_pairwise``);
addPoseToGraph hangs the converted information on a measured loop closure of a ``capi.PoseGraph``.

Two additions of ours: the target's normals are estimated (knn 30) when it has none -- the prototype never estimates
them and Open3D would refuse such a cloud -- and the 6 x 6 matrix is converted to the graph's error coordinates
(``icp_edge_information``) before it is stored."""
from __future__ import annotations

import numpy as np

from . import capi


class PoseGraphOptimize:
    def __init__(self, ctx: capi.Context, pose_graph: capi.PoseGraph | None = None, downSampleFactor: float = 1.0,
                 knn: int = 30, **icp_params):
        self.ctx = ctx
        self.downSampleFactor = downSampleFactor
        self.max_correspondence_distance_coarse = downSampleFactor * 15
        self.max_correspondence_distance_fine = downSampleFactor * 1.5
        self.knn = knn
        self.icp_params = icp_params
        self.poseGraph = pose_graph if pose_graph is not None else capi.PoseGraph(ctx)

    def _target(self, target) -> capi.Cloud:
        cloud = target if isinstance(target, capi.Cloud) else capi.Cloud(self.ctx, target)
        if not cloud.has_normals:
            cloud.estimate_normals(self.knn)
        return cloud

    def pairwiseRegistration(self, source, target):
        """source: n x 3 float32 points; target: the same or a ``capi.Cloud`` -> (T [4, 4], Lambda [6, 6]); T maps source
        coordinates into the target's frame."""
        T, info, _ = self.ctx.icp_pairwise(source, self._target(target), self.max_correspondence_distance_coarse,
                                           self.max_correspondence_distance_fine, **self.icp_params)
        return T, info

    def addPoseToGraph(self, source, target, R=None, t=None, fromNodeID=None, toNodeID=None, loopClosure=True,
                       loopClosureNode=None):
        """A measured loop closure: the edge (newest vertex -> vertex ``loopClosureNode``, else ``toNodeID``) with the
        measurement T = X_newest^-1 X_matched and its information.  source = the matched keyframe's cloud, target = the
        newest frame's, each in its own camera frame.  With R, t given (the prototype's call) T = [R | t] and the
        information is taken at the coarse distance, as the prototype does; without them both come from
        pairwiseRegistration.  Odometry edges are ``PoseGraph.augment_node``'s and are not added here.
        -> (T, Lambda, info21)"""
        if not loopClosure:
            raise ValueError("odometry edges come from PoseGraph.augment_node; addPoseToGraph adds loop closures")
        node = loopClosureNode if loopClosureNode is not None else toNodeID
        if node is None:
            raise ValueError("the matched vertex is needed: loopClosureNode or toNodeID")
        if R is None:
            T, info = self.pairwiseRegistration(source, target)
        else:
            T = np.eye(4)
            T[:3, :3] = np.asarray(R, np.float64).reshape(3, 3)
            T[:3, 3] = np.asarray(t, np.float64).reshape(3)
            info, _ = self.ctx.icp_information(source, self._target(target), self.max_correspondence_distance_coarse, T)
        info21 = capi.icp_edge_information(info, T)
        self.poseGraph.add_loop_closure(int(node), capi.icp_meas7(T), info21)
        return T, info, info21
