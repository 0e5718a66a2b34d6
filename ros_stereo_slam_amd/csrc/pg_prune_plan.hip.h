// pg_prune_plan.hip.h -- the host arithmetic of the pose graph's robust kernels and of svo_pg_prune_edges with nothing of HIP in it:
// which (kind, delta) pairs are refused, which edges a prune removes, the remap of the edges that stay, the reachability test and the
// two refusals.  posegraph.hip includes it; so does tests/cpp/pg_prune_plan_check.cpp, a stand-alone program that runs it under the
// address and undefined-behaviour sanitizers.
#pragma once

#include <cmath>
#include <cstddef>
#include <vector>

#include "../../include/svo.h"

namespace pg_prune_plan {

// what svo_pg_set_robust_kernel and svo_pg_set_loop_closure_kernel refuse; 0, or the reason.  NONE takes any delta (it is not read);
// `delta > 0` is false for a NaN.
inline const char *check_kernel(int kind, double delta)
{
    if (kind < SVO_PG_ROBUST_NONE || kind > SVO_PG_ROBUST_GEMAN_MCCLURE)
        return "unknown robust kernel";
    if (kind != SVO_PG_ROBUST_NONE && !(delta > 0.0 && std::isfinite(delta)))
        return "the kernel's parameter must be finite and positive";
    return nullptr;
}

enum { PRUNE_OK = 0, PRUNE_CAPACITY = 1, PRUNE_DISCONNECTS = 2 };

struct Plan {
    std::vector<int> removed;  // former indices, ascending
    std::vector<int> remap;    // [ne]: an edge's new index, -1 for a removed one
    int orphan = -1;           // PRUNE_DISCONNECTS: the lowest vertex the removal would cut off from vertex 0
};

inline int uf_find(std::vector<int> &parent, int v)
{
    while (parent[v] != v) {
        parent[v] = parent[parent[v]];  // path halving
        v = parent[v];
    }
    return v;
}

// An edge goes when it carries a kernel (kind[e] != NONE; kind == nullptr: no edge does), joins two vertices that are not consecutive
// and has weight[e] < threshold (strict; false for a NaN on either side).  Nothing is changed here: the caller applies `remap` only
// after PRUNE_OK.  cap: the slots of the caller's `removed` array.
inline int plan(int nv, int ne, const int *efrom, const int *eto, const int *kind, const double *weight, double threshold, int cap,
                Plan &out)
{
    out.removed.clear();
    out.remap.assign(ne > 0 ? (size_t)ne : 0, -1);
    out.orphan = -1;
    for (int e = 0; e < ne; e++) {
        const int d = efrom[e] - eto[e];
        if (kind && kind[e] != SVO_PG_ROBUST_NONE && d != 1 && d != -1 && weight[e] < threshold)
            out.removed.push_back(e);
    }
    if ((long long)out.removed.size() > (long long)(cap > 0 ? cap : 0))
        return PRUNE_CAPACITY;
    std::vector<int> parent(nv > 0 ? (size_t)nv : 0);
    for (int v = 0; v < nv; v++)
        parent[v] = v;
    size_t r = 0;
    int kept = 0;
    for (int e = 0; e < ne; e++) {
        if (r < out.removed.size() && out.removed[r] == e) {
            r++;
            continue;
        }
        out.remap[e] = kept++;
        const int a = uf_find(parent, efrom[e]), b = uf_find(parent, eto[e]);
        if (a != b)
            parent[a > b ? a : b] = a > b ? b : a;  // the lower vertex is the root: vertex 0 stays the root of its component
    }
    if (!out.removed.empty())
        for (int v = 1; v < nv; v++)
            if (uf_find(parent, v) != 0) {
                out.orphan = v;
                return PRUNE_DISCONNECTS;
            }
    return PRUNE_OK;
}

// moves the records (`stride` values each) of the edges that stay to their new places, in order, and cuts the tail off
template <typename T>
inline void compact(std::vector<T> &v, size_t stride, const std::vector<int> &remap)
{
    size_t kept = 0;
    for (size_t e = 0; e < remap.size(); e++) {
        if (remap[e] < 0)
            continue;
        if ((size_t)remap[e] != e)
            for (size_t k = 0; k < stride; k++)
                v[stride * (size_t)remap[e] + k] = v[stride * e + k];
        kept++;
    }
    v.resize(stride * kept);
}

}  // namespace pg_prune_plan
