// pg_g2o_check.cpp -- the pose graph's reader of .g2o files and its test of an information matrix (csrc/pg_g2o.hip.h) exercised on
// their own: files written to a temporary directory, the parsed content or the exact text of the refusal asserted;
// tests/test_pg_plan_abi.py builds it with -fsanitize=address,undefined and runs it.  No GPU.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include <unistd.h>

#include "../../ros_stereo_slam_amd/csrc/pg_g2o.hip.h"

using namespace pg_g2o;

#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            return 1;                                                         \
        }                                                                     \
    } while (0)

static std::string g_path;

static bool write_file(const std::string &text)
{
    FILE *f = fopen(g_path.c_str(), "w");
    if (!f)
        return false;
    const bool ok = fwrite(text.data(), 1, text.size(), f) == text.size();
    return fclose(f) == 0 && ok;
}

// the refusal of a file with this content ("" = accepted), as the text after the path
static std::string refusal(const std::string &text, bool keep_info, Graph &g)
{
    if (!write_file(text))
        return "cannot write the file";
    const std::string why = read(g_path.c_str(), keep_info, g);
    if (why.empty())
        return why;
    return why.compare(0, g_path.size(), g_path) == 0 ? why.substr(g_path.size()) : "no path in front: " + why;
}

static std::string numbers(const std::vector<double> &v)
{
    std::string s;
    for (double x : v)
        s += format(" %.17g", x);
    return s;
}

int main(int argc, char **argv)  // [the directory to make the temporary one in]
{
    std::string dir_name = std::string(argc > 1 ? argv[1] : "/tmp") + "/pg_g2o_check_XXXXXX";
    char *dir = &dir_name[0];
    EXPECT(mkdtemp(dir));
    g_path = dir_name + "/graph.g2o";
    const double nan = std::nan(""), inf = std::numeric_limits<double>::infinity();
    const std::vector<double> identity(INFO_IDENTITY, INFO_IDENTITY + 21);
    Graph g;

    // check_info: the triangle's order, the two refusals
    static_assert(pg_tri(0, 0) == 0 && pg_tri(0, 5) == 5 && pg_tri(1, 1) == 6 && pg_tri(5, 1) == 10 && pg_tri(2, 2) == 11 &&
                      pg_tri(4, 5) == 19 && pg_tri(5, 5) == 20, "upper triangle, row-major");
    {
        std::vector<double> om = identity;
        EXPECT(check_info(om.data(), "edge", 3).empty());
        om[pg_tri(0, 1)] = 0.999;  // [[1, .999], [.999, 1]] is positive definite, with 1.0 it is singular
        EXPECT(check_info(om.data(), "edge", 3).empty());
        om[pg_tri(0, 1)] = 1.0;
        EXPECT(check_info(om.data(), "edge", 3) == "pose graph: edge 3: information matrix is not positive definite (pivot 1 = 0)");
        om[pg_tri(0, 1)] = 0, om[20] = -inf;
        EXPECT(check_info(om.data(), "new edge", 0) == "pose graph: new edge 0: information entry 20 is not finite");
        om[20] = 1, om[0] = nan;
        EXPECT(check_info(om.data(), "new edge", 7) == "pose graph: new edge 7: information entry 0 is not finite");
        om[0] = 0;
        EXPECT(check_info(om.data(), "edge", 0) == "pose graph: edge 0: information matrix is not positive definite (pivot 0 = 0)");
    }

    // a round trip: three vertices (one quaternion not normalised), three edges: 21 numbers, none, the identity's 21
    std::vector<double> om2(21, 0.);
    for (int i = 0; i < 6; i++)
        om2[pg_tri(i, i)] = 2 + i;
    om2[pg_tri(0, 3)] = 0.25;
    const std::string verts3 = "VERTEX_SE3:QUAT 0 0 0 0 0 0 0 1\nVERTEX_SE3:QUAT 1 1 0 0 0 0 0 2\nVERTEX_SE3:QUAT 2 2 0.5 0 0 0 0 1\n";
    const std::string edges3 = "EDGE_SE3:QUAT 0 1 1 0 0 0 0 0 1" + numbers(om2) + "\nEDGE_SE3:QUAT 1 2 1 0.5 0 0 0 0 1\n" +
                               "EDGE_SE3:QUAT 2 0 -2 -0.5 0 0 3 0 4" + numbers(identity) + "\n";
    for (int keep = 0; keep < 2; keep++) {
        EXPECT(refusal(verts3 + edges3, keep, g).empty());
        EXPECT(g.pose == std::vector<double>({0, 0, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 1, 2, 0.5, 0, 0, 0, 0, 1}));
        EXPECT(g.efrom == std::vector<int>({0, 1, 2}) && g.eto == std::vector<int>({1, 2, 0}));
        EXPECT(g.meas == std::vector<double>({1, 0, 0, 0, 0, 0, 1, 1, 0.5, 0, 0, 0, 0, 1, -2, -0.5, 0, 0, 0.6, 0, 0.8}));
        if (keep) {
            std::vector<double> all = om2;
            all.insert(all.end(), identity.begin(), identity.end());
            all.insert(all.end(), identity.begin(), identity.end());
            EXPECT(g.has_info == std::vector<char>({1, 0, 1}) && g.info == all);
        } else
            EXPECT(g.has_info.empty() && g.info.empty());
    }
    // comments, unknown tags, blank lines, FIX 0, carriage returns; vertices out of order; a last line without a newline
    EXPECT(refusal("# a comment\n\n   \nFOO 1 2 3\nVERTEX_SE3:QUAT 2 2 0 0 0 0 0 1\r\n#VERTEX_SE3:QUAT 7 0 0 0 0 0 0 1\nVERTEX_SE3:QUAT 0 0 0 0 0 0 0 1\n"
                   "FIX 0\nVERTEX_TRACKXYZ 5 1 2 3\nVERTEX_SE3:QUAT 1 1 0 0 0 0 0 1\nEDGE_SE3:QUAT 1 2 1 0 0 0 0 0 1 \t\r\nEDGE_SE3:QUAT 0 1 1 0 0 0 0 0 1",
                   true, g).empty());
    EXPECT(g.pose == std::vector<double>({0, 0, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 1, 2, 0, 0, 0, 0, 0, 1}));
    EXPECT(g.efrom == std::vector<int>({1, 0}) && g.eto == std::vector<int>({2, 1}) && g.has_info == std::vector<char>({0, 0}));
    EXPECT(g.info.size() == 42 && g.meas.size() == 14 && g.meas[7] == 1 && g.meas[13] == 1);

    const std::string v2 = "VERTEX_SE3:QUAT 0 0 0 0 0 0 0 1\nVERTEX_SE3:QUAT 1 1 0 0 0 0 0 1\n", e01 = "EDGE_SE3:QUAT 0 1 1 0 0 0 0 0 1";
    // the vertex ids
    EXPECT(refusal(v2 + "VERTEX_SE3:QUAT 1 1 0 0 0 0 0 1\n", false, g) == ": vertex ids must be 0..2 without gaps or repeats (id 1)");
    EXPECT(refusal("VERTEX_SE3:QUAT 0 0 0 0 0 0 0 1\nVERTEX_SE3:QUAT 2 1 0 0 0 0 0 1\n", false, g) ==
           ": vertex ids must be 0..1 without gaps or repeats (id 2)");
    EXPECT(refusal("VERTEX_SE3:QUAT 0 0 0 0 0 0 0 1\nVERTEX_SE3:QUAT -1 1 0 0 0 0 0 1\n", false, g) == ":2: malformed VERTEX_SE3:QUAT");
    EXPECT(refusal("VERTEX_SE3:QUAT 0 0 0 0 0 0 0\n", false, g) == ":1: malformed VERTEX_SE3:QUAT");
    EXPECT(refusal("VERTEX_SE3:QUAT", false, g) == ":1: malformed VERTEX_SE3:QUAT");
    // the edges' vertices
    EXPECT(refusal(v2 + "EDGE_SE3:QUAT 0 5 1 0 0 0 0 0 1\n", false, g) == ": edge 0 connects vertices 0 -> 5 of 2");
    EXPECT(refusal(v2 + e01 + "\nEDGE_SE3:QUAT -1 0 1 0 0 0 0 0 1\n", false, g) == ": edge 1 connects vertices -1 -> 0 of 2");
    EXPECT(refusal(v2 + "EDGE_SE3:QUAT 1 1 1 0 0 0 0 0 1\n", true, g) == ": edge 0 connects vertices 1 -> 1 of 2");
    EXPECT(refusal(v2 + "EDGE_SE3:QUAT 0 1 1 0 0 0 0 x 1\n", false, g) == ":3: malformed EDGE_SE3:QUAT");
    EXPECT(refusal(e01 + "\n", false, g) == ": edge 0 connects vertices 0 -> 1 of 0");
    // FIX
    EXPECT(refusal(v2 + "FIX 1\n", false, g) == ":3: only vertex 0 can be fixed (FIX 1)");
    EXPECT(refusal("FIX\n" + v2, false, g) == ":1: only vertex 0 can be fixed (FIX -1)");
    // the information numbers: 0 or 21, nothing after them; without keep_info they are not looked at
    std::vector<double> om20(identity.begin(), identity.begin() + 20), om22 = identity;
    om22.push_back(1);
    EXPECT(refusal(v2 + e01 + numbers(om20) + "\n", true, g) == ":3: EDGE_SE3:QUAT with 20 information numbers (0 or 21 expected)");
    EXPECT(refusal(v2 + e01 + numbers(om22) + "\n", true, g) == ":3: EDGE_SE3:QUAT with 22 information numbers (0 or 21 expected)");
    EXPECT(refusal(v2 + e01 + numbers(std::vector<double>(40, 1.)) + "\n", true, g) ==
           ":3: EDGE_SE3:QUAT with 40 information numbers (0 or 21 expected)");
    EXPECT(refusal(v2 + e01 + numbers(identity) + " junk\n", true, g) == ":3: EDGE_SE3:QUAT with 21 information numbers (0 or 21 expected)");
    EXPECT(refusal(v2 + e01 + " junk\n", true, g) == ":3: EDGE_SE3:QUAT with 0 information numbers (0 or 21 expected)");
    EXPECT(refusal(v2 + e01 + numbers(om20) + " junk\n", false, g).empty() && g.efrom.size() == 1 && g.info.empty());
    // ... finite and positive definite
    std::vector<double> bad = identity;
    bad[3] = nan;
    EXPECT(refusal(v2 + e01 + numbers(bad) + "\n", true, g) == ":3: pose graph: edge 0: information entry 3 is not finite");
    bad[3] = 0, bad[20] = inf;
    EXPECT(refusal(v2 + "\n" + e01 + "\n" + e01 + numbers(bad) + "\n", true, g) == ":5: pose graph: edge 1: information entry 20 is not finite");
    bad[20] = 1, bad[pg_tri(2, 2)] = -1;
    EXPECT(refusal(v2 + e01 + numbers(bad) + "\n", true, g) ==
           ":3: pose graph: edge 0: information matrix is not positive definite (pivot 2 = -1)");
    EXPECT(refusal(v2 + e01 + numbers(bad) + "\n", false, g).empty());
    // no vertices, nothing at all, no file
    EXPECT(refusal("# nothing\nFIX 0\n", true, g) == ": no VERTEX_SE3:QUAT lines");
    EXPECT(refusal("", true, g) == ": no VERTEX_SE3:QUAT lines");
    // a line is read in pieces of 4095 bytes: the rest of a long comment is a line of its own, here an unknown tag, and is counted
    EXPECT(refusal("#" + std::string(5000, 'x') + "\n" + v2 + "FIX 3\n", false, g) == ":5: only vertex 0 can be fixed (FIX 3)");
    // ... and the numbers of a long edge line that the cut leaves to the next piece are not this edge's
    EXPECT(refusal(v2 + "EDGE_SE3:QUAT 0 1 1 0 0 0 0 0 1" + std::string(4064, ' ') + numbers(identity) + "\n", true, g).empty());
    EXPECT(g.efrom.size() == 1 && g.has_info == std::vector<char>({0}));
    EXPECT(refusal(std::string(100, 'T') + " 1 2\n" + v2, false, g).empty() && g.pose.size() == 14);
    EXPECT(unlink(g_path.c_str()) == 0);
    EXPECT(read(g_path.c_str(), true, g) == "cannot open " + g_path);
    EXPECT(rmdir(dir) == 0);
    std::puts("pg g2o check ok");
    return 0;
}
