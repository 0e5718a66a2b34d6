// pg_g2o.hip.h -- what the pose graph does with input from outside the process, with nothing of HIP in it: the test an information
// matrix has to pass (finite, positive definite by a host 6 x 6 Cholesky) and the reader of .g2o files, both with the reasons of
// their refusals as text.  posegraph.hip includes it, turns a reason into svo_set_error and commits a parsed graph; so does
// tests/cpp/pg_g2o_check.cpp, a stand-alone program that runs it under the address and undefined-behaviour sanitizers.
// pg_tri and q_normalize are here because the reader and the kernels both need them.
#pragma once

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#ifdef __HIPCC__  // as FAST_PLAN_HD of fast_plan.hip.h
#define PG_G2O_HD __host__ __device__
#else
#define PG_G2O_HD
#endif

namespace pg_g2o {

// Index of entry (i, j), i <= j, of a symmetric 6 x 6 matrix stored as its upper triangle, row-major (g2o's order)
PG_G2O_HD constexpr int pg_tri(int i, int j)
{
    const int a = i <= j ? i : j, b = i <= j ? j : i;
    return 6 * a - a * (a - 1) / 2 + (b - a);
}

PG_G2O_HD inline void q_normalize(double *q)
{
    const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    if (n > 0)
        for (int i = 0; i < 4; i++)
            q[i] /= n;
}

constexpr double INFO_IDENTITY[21] = {1, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 1, 0, 1};

// printf into a string of whatever length it takes (a path has no bound here; svo_set_error cuts at its own)
#if defined(__GNUC__)
__attribute__((format(printf, 1, 2)))
#endif
inline std::string format(const char *fmt, ...)
{
    va_list ap, ap2;
    va_start(ap, fmt);
    va_copy(ap2, ap);
    const int n = vsnprintf(nullptr, 0, fmt, ap);
    va_end(ap);
    std::string s(n > 0 ? (size_t)n : 0, '\0');
    if (n > 0)
        vsnprintf(&s[0], (size_t)n + 1, fmt, ap2);
    va_end(ap2);
    return s;
}

// A usable information matrix is finite and positive definite (host 6 x 6 Cholesky: every pivot > 0); `what` names the edge.
// "" or the reason.
inline std::string check_info(const double *info21, const char *what, int e)
{
    for (int k = 0; k < 21; k++)
        if (!std::isfinite(info21[k]))
            return format("pose graph: %s %d: information entry %d is not finite", what, e, k);
    double L[36];
    for (int i = 0; i < 6; i++)
        for (int j = 0; j <= i; j++) {
            double v = info21[pg_tri(j, i)];
            for (int k = 0; k < j; k++)
                v -= L[6 * i + k] * L[6 * j + k];
            if (i == j) {
                if (!(v > 0))
                    return format("pose graph: %s %d: information matrix is not positive definite (pivot %d = %g)", what, e, i, v);
                L[6 * i + i] = sqrt(v);
            } else
                L[6 * i + j] = v / L[6 * j + j];
        }
    return std::string();
}

struct Graph {
    std::vector<double> pose;  // 7 per vertex, quaternions normalised
    std::vector<int> efrom, eto;
    std::vector<double> meas;    // 7 per edge, quaternions normalised
    std::vector<double> info;    // keep_info: 21 per edge, the identity's numbers where the file has none; else empty
    std::vector<char> has_info;  // keep_info: one per edge; else empty
};

/* The inverse of svo_pg_write_g2o / saveStructure: the file's content -> out; "" or the reason of the refusal (out is then
 * unspecified).  Tags read: VERTEX_SE3:QUAT id x y z qx qy qz qw, EDGE_SE3:QUAT i j x y z qx qy qz qw [21 numbers of
 * the upper-triangular information matrix; without keep_info ignored: the reference leaves it at identity,
 * poseGraph.h:102-104,122], FIX id (only vertex 0 may be fixed, as upstream fixes it, :75).  Vertex
 * ids must be 0..n-1 (any order in the file); other tags are skipped.  A line is read in pieces of 4095 bytes: what lies
 * beyond is taken as lines of its own (and counted as such).                                                           */
inline std::string read(const char *path, const bool keep_info, Graph &out)
{
    FILE *f = fopen(path, "r");
    if (!f)
        return format("cannot open %s", path);
    std::vector<std::pair<int, std::vector<double>>> verts;
    out = Graph();
    std::string why;
    char line[4096], tag[64];
    int lineno = 0;
    while (why.empty() && fgets(line, sizeof(line), f)) {
        lineno++;
        int off = 0;
        if (sscanf(line, "%63s%n", tag, &off) != 1 || tag[0] == '#')
            continue;
        const char *rest = line + off;
        if (!strcmp(tag, "VERTEX_SE3:QUAT")) {
            int id;
            double p[7];
            if (sscanf(rest, "%d %lf %lf %lf %lf %lf %lf %lf", &id, p, p + 1, p + 2, p + 3, p + 4, p + 5, p + 6) != 8 || id < 0) {
                why = format("%s:%d: malformed VERTEX_SE3:QUAT", path, lineno);
                break;
            }
            q_normalize(p + 3);
            verts.emplace_back(id, std::vector<double>(p, p + 7));
        } else if (!strcmp(tag, "EDGE_SE3:QUAT")) {
            int i, j, used = 0;
            double z[7];
            if (sscanf(rest, "%d %d %lf %lf %lf %lf %lf %lf %lf%n", &i, &j, z, z + 1, z + 2, z + 3, z + 4, z + 5, z + 6, &used) != 9) {
                why = format("%s:%d: malformed EDGE_SE3:QUAT", path, lineno);
                break;
            }
            if (keep_info) {  // none (identity) or exactly the 21 numbers of the upper triangle
                double om[22];
                int cnt = 0;
                const char *c = rest + used;
                for (;;) {
                    char *end = nullptr;
                    const double v = strtod(c, &end);
                    if (end == c)
                        break;
                    if (cnt < 22)
                        om[cnt] = v;
                    cnt++;
                    c = end;
                }
                while (*c == ' ' || *c == '\t' || *c == '\r' || *c == '\n')
                    c++;
                if ((cnt != 0 && cnt != 21) || *c) {
                    why = format("%s:%d: EDGE_SE3:QUAT with %d information numbers (0 or 21 expected)", path, lineno, cnt);
                    break;
                }
                if (cnt == 21) {
                    const std::string bad = check_info(om, "edge", (int)out.efrom.size());
                    if (!bad.empty()) {
                        why = format("%s:%d: %s", path, lineno, bad.c_str());
                        break;
                    }
                }
                out.has_info.push_back(cnt == 21);
                out.info.insert(out.info.end(), cnt == 21 ? om : INFO_IDENTITY, (cnt == 21 ? om : INFO_IDENTITY) + 21);
            }
            q_normalize(z + 3);
            out.efrom.push_back(i);
            out.eto.push_back(j);
            out.meas.insert(out.meas.end(), z, z + 7);
        } else if (!strcmp(tag, "FIX")) {
            int id = -1;
            if (sscanf(rest, "%d", &id) != 1 || id != 0)
                why = format("%s:%d: only vertex 0 can be fixed (FIX %d)", path, lineno, id);
        }
    }
    fclose(f);
    if (!why.empty())
        return why;
    const int n = (int)verts.size();
    out.pose.assign((size_t)n * 7, 0.);
    std::vector<char> seen(n, 0);
    for (auto &v : verts) {
        if (v.first >= n || seen[v.first])
            return format("%s: vertex ids must be 0..%d without gaps or repeats (id %d)", path, n - 1, v.first);
        seen[v.first] = 1;
        memcpy(&out.pose[(size_t)v.first * 7], v.second.data(), 7 * sizeof(double));
    }
    for (size_t e = 0; e < out.efrom.size(); e++)
        if (out.efrom[e] < 0 || out.efrom[e] >= n || out.eto[e] < 0 || out.eto[e] >= n || out.efrom[e] == out.eto[e])
            return format("%s: edge %zu connects vertices %d -> %d of %d", path, e, out.efrom[e], out.eto[e], n);
    if (n == 0)
        return format("%s: no VERTEX_SE3:QUAT lines", path);
    return std::string();
}

}  // namespace pg_g2o
