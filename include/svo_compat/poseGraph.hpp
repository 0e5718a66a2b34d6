// svo_compat/poseGraph.hpp -- the reference's globalPoseGraph (include/poseGraph.h:36-179) on
// top of the svo_pg_* C ABI.  Same method names, argument meaning and side effects
// (result.g2o written by globalOptimize, poseGraph.g2o by saveStructure); no g2o, no Eigen
// required (see types.hpp for the Isometry3d stand-in / binding).
#pragma once

#include "types.hpp"

namespace svo_compat {

// The 6 x 6 `information` member (Eigen::Matrix<double, 6, 6> upstream, include/poseGraph.h:42): identity by default,
// element access M(r, c) as Eigen's -- an Eigen matrix is copied into it entry by entry.
struct Matrix6d {
    double m[36] = {1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1};
    static Matrix6d Identity() { return Matrix6d(); }
    double &operator()(int r, int c) { return m[6 * r + c]; }
    double operator()(int r, int c) const { return m[6 * r + c]; }
};

class globalPoseGraph {
  public:
    int globalNodeID = 0;          // include/poseGraph.h:38
    bool loopClosureFlag = false;  // :39
    // :42 -- the information matrix of new edges, in g2o's order (translation, then the quaternion's vector part).  The
    // reference declares it and leaves its setInformation(information) calls commented out (:103,122): applied to the edges
    // augmentNode / addLoopClosure add only when INFORMATION_FLAG is set.
    Matrix6d information = Matrix6d::Identity();
    bool INFORMATION_FLAG = false;
    // true: addLoopClosure(T, fromID) uses T as the edge's measurement (what getLCMeasurement, dump.cpp:331-348, produces);
    // false: the reference's behaviour, T is never read and the measurement is the identity
    bool MEASURED_LC_FLAG = false;
    std::string outFileName = "poseGraph.g2o";  // :56
    int optimizeIterations = 10;   // optimizer.optimize(10), :130
    bool writeResultFile = true;   // optimizer.save("result.g2o"), :131

    explicit globalPoseGraph(svo_ctx *ctx = nullptr) : ctx_(ctx ? ctx : shared_context()) { check(svo_pg_create(ctx_, &pg_)); }
    ~globalPoseGraph() { svo_pg_destroy(pg_); }
    globalPoseGraph(const globalPoseGraph &) = delete;
    globalPoseGraph &operator=(const globalPoseGraph &) = delete;

    // :69-84 -- vertex 0 = identity, fixed
    void initializeGraph()
    {
        check(svo_pg_initialize(pg_));
        globalNodeID = 1;
    }
    // :87-111 -- localT is never read by the reference either
    void augmentNode(const Isometry3d & /*localT*/, const Isometry3d &globalT)
    {
        double p[7];
        iso_to_pose7(globalT, p);
        check(svo_pg_augment_node(pg_, p));
        if (INFORMATION_FLAG) {  // edge->setInformation(information), :103
            double om[21];
            info21(om);
            check(svo_pg_set_edge_information(pg_, svo_pg_num_edges(pg_) - 1, om));
        }
        globalNodeID++;
    }
    // :113-126 -- T is unused by the reference (the measurement is the identity) unless MEASURED_LC_FLAG is set
    void addLoopClosure(const Isometry3d &T, int fromID)
    {
        if (!MEASURED_LC_FLAG && !INFORMATION_FLAG)
            check(svo_pg_add_loop_closure(pg_, fromID));
        else {
            double z[7], om[21];
            if (MEASURED_LC_FLAG)
                iso_to_pose7(T, z);
            if (INFORMATION_FLAG)
                info21(om);
            check(svo_pg_add_loop_closure_measured(pg_, fromID, MEASURED_LC_FLAG ? z : nullptr, INFORMATION_FLAG ? om : nullptr));
        }
        loopClosureFlag = true;
    }
    // :128-138 -- 10 Gauss-Newton iterations over the whole graph, every estimate returned
    std::vector<Isometry3d> globalOptimize()
    {
        check(svo_pg_optimize(pg_, optimizeIterations, nullptr));
        if (writeResultFile)
            check(svo_pg_write_g2o(pg_, "result.g2o"));
        return estimates();
    }
    std::vector<Isometry3d> estimates() const
    {
        const int n = svo_pg_num_vertices(pg_);
        std::vector<double> p((size_t)n * 7);
        check(svo_pg_get_estimates(pg_, p.data()));
        std::vector<Isometry3d> out;
        out.reserve(n);
        for (int i = 0; i < n; i++)
            out.push_back(pose7_to_iso(&p[7 * i]));
        return out;
    }
    // Not in the reference, off by default: the robust kernel (SVO_PG_ROBUST_*, include/svo.h) of every loop closure that
    // addLoopClosure adds from now on; SVO_PG_ROBUST_NONE brings the reference's behaviour back.
    void setLoopClosureKernel(int kind, double delta) { check(svo_pg_set_loop_closure_kernel(pg_, kind, delta)); }
    // Not in the reference: removes the closures whose robust weight at the current estimates is below `threshold`
    // (svo_pg_prune_edges) and returns their former edge indices, ascending.
    std::vector<int> pruneLoopClosures(double threshold)
    {
        std::vector<int> removed((size_t)svo_pg_num_edges(pg_) + 1);
        int n = 0;
        check(svo_pg_prune_edges(pg_, threshold, removed.data(), (int)removed.size(), &n));
        removed.resize((size_t)n);
        return removed;
    }
    // :140-179
    void saveStructure() { check(svo_pg_write_g2o(pg_, outFileName.c_str())); }
    int numVertices() const { return svo_pg_num_vertices(pg_); }
    int numEdges() const { return svo_pg_num_edges(pg_); }
    svo_posegraph *handle() { return pg_; }

  private:
    // the upper triangle of `information`, row-major: what the C ABI and an EDGE_SE3:QUAT line carry
    void info21(double *om) const
    {
        int k = 0;
        for (int i = 0; i < 6; i++)
            for (int j = i; j < 6; j++)
                om[k++] = information(i, j);
    }
    svo_ctx *ctx_;
    svo_posegraph *pg_ = nullptr;
};

}  // namespace svo_compat
