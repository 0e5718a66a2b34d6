"""PoseGraphOptimize of the Python prototype (src/ROSslam.py:34-73) on the library's own ICP: pairwiseRegistration is a
coarse and a fine point-to-plane registration and the information matrix at the fine distance (``svo_icp_pairwise``);
addPoseToGraph hangs the converted information on a measured loop closure of a ``capi.PoseGraph``.

With ``voxel_down_sample=True`` array sources and array targets first pass through ``svo_voxel_downsample`` at
``downSampleFactor``, the voxel size the recipe's two distances are stated in; the default does not.

Two additions of ours: the target's normals are estimated (knn 30) when it has none -- the prototype never estimates
them and Open3D would refuse such a cloud -- and the 6 x 6 matrix is converted to the graph's error coordinates
(``icp_edge_information``) before it is stored.

``globalOptimize`` stands in for Open3D's global optimisation of that graph: the closures addPoseToGraph added are the
prototype's ``uncertain`` edges, carry the line process (the Geman-McClure kernel) and are pruned below a weight."""
from __future__ import annotations

import numpy as np

from . import capi


class PoseGraphOptimize:
    def __init__(self, ctx: capi.Context, pose_graph: capi.PoseGraph | None = None, downSampleFactor: float = 1.0,
                 knn: int = 30, voxel_down_sample: bool = False, **icp_params):
        self.ctx = ctx
        self.downSampleFactor = downSampleFactor
        # Open3D's recipe passes both clouds through voxel_down_sample(voxel_size = downSampleFactor) before estimate_normals and
        # registration_icp, which is what the two distances below are stated in; off by default: every earlier call keeps its bits
        self.voxel_down_sample = bool(voxel_down_sample)
        self.max_correspondence_distance_coarse = downSampleFactor * 15
        self.max_correspondence_distance_fine = downSampleFactor * 1.5
        self.knn = knn
        self.icp_params = icp_params
        self.poseGraph = pose_graph if pose_graph is not None else capi.PoseGraph(ctx)
        # the closures addPoseToGraph added, Open3D's `uncertain` edges: (from, to, correspondence count), in the graph's edge order
        self.uncertain: list[tuple[int, int, float]] = []

    def _thinned(self, cloud):
        """an array cloud through ``voxel_downsample`` at downSampleFactor when voxel_down_sample is set; a ``capi.Cloud`` as given"""
        if not self.voxel_down_sample or isinstance(cloud, capi.Cloud):
            return cloud
        return self.ctx.voxel_downsample(cloud, self.downSampleFactor)[0]

    def _target(self, target) -> capi.Cloud:
        cloud = target if isinstance(target, capi.Cloud) else capi.Cloud(self.ctx, self._thinned(target))
        if not cloud.has_normals:
            cloud.estimate_normals(self.knn)
        return cloud

    def pairwiseRegistration(self, source, target):
        """source: n x 3 float32 points; target: the same or a ``capi.Cloud`` -> (T [4, 4], Lambda [6, 6]); T maps source
        coordinates into the target's frame."""
        T, info, _ = self.ctx.icp_pairwise(self._thinned(source), self._target(target), self.max_correspondence_distance_coarse,
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
            info, _ = self.ctx.icp_information(self._thinned(source), self._target(target), self.max_correspondence_distance_coarse, T)
        info21 = capi.icp_edge_information(info, T)
        newest = self.poseGraph.num_vertices - 1
        self.poseGraph.add_loop_closure(int(node), capi.icp_meas7(T), info21)
        # the prototype adds it as PoseGraphEdge(..., uncertain=True) (src/ROSslam.py:57).  Lambda = sum G^T G with G = [-[t]x | I3]
        # per correspondence (svo_icp_information), so Lambda(5, 5) is the number of correspondences
        self.uncertain.append((newest, int(node), float(np.asarray(info, np.float64).reshape(6, 6)[5, 5])))
        return T, info, info21

    def _uncertain_edges(self):
        """the graph's edge index of every recorded closure that is still in the graph, matched in order by its end points"""
        want = list(self.uncertain)
        out = []
        for e, (i, j, _) in enumerate(self.poseGraph.edges()):
            if want and (i, j) == want[0][:2] and abs(i - j) != 1:
                out.append((e, want.pop(0)))
        if want:
            raise RuntimeError(f"closures {[w[:2] for w in want]} are no longer in the graph in the order they were added")
        return out

    def globalOptimize(self, iters: int = 10, preference_loop_closure: float = 1.0, edge_prune_threshold: float = 0.25):
        """Open3D's global optimisation of the prototype's graph, on this library's solver: every closure addPoseToGraph added
        carries the line process -- the Geman-McClure kernel with mu = preference_loop_closure *
        max_correspondence_distance_fine^2 * (mean correspondence count of those closures), Open3D's ComputeLineProcessWeight
        AS RECALLED, to be verified --; the graph is optimised, the closures whose weight l = (mu / (mu + chi2))^2 is below
        edge_prune_threshold are removed, and the graph is optimised again.
        Deviations: chi2 is the graph's own e^T Omega e with Omega from ``icp_edge_information``, not Open3D's misalignment
        vector; the solver is Gauss-Newton, not Levenberg-Marquardt.
        -> the removed closures as (from, to, correspondence count)"""
        closures = self._uncertain_edges()
        if not closures:
            self.poseGraph.optimize(iters)
            return []
        mu = float(preference_loop_closure) * self.max_correspondence_distance_fine ** 2 * float(np.mean([c[2] for _, c in closures]))
        for e, _ in closures:
            self.poseGraph.set_robust_kernel(e, capi.PG_ROBUST_GEMAN_MCCLURE, mu)
        self.poseGraph.optimize(iters)
        gone = set(int(e) for e in self.poseGraph.prune_edges(edge_prune_threshold))
        removed = [c for e, c in closures if e in gone]
        self.uncertain = [c for e, c in closures if e not in gone]
        if removed:
            self.poseGraph.optimize(iters)
        return removed
