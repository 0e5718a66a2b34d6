// pg_solve_plan_check.cpp -- the elimination structure of the pose graph's solve (csrc/pg_solve_plan.hip.h: separators, segments,
// couplings, the gather lists and the one int buffer the kernels index) built for a set of graphs under each structure (both ends,
// the cover, the cost model's choice) and every index in it checked against the bounds of what a kernel reads with it;
// tests/test_pg_plan_abi.py builds it with -fsanitize=address,undefined and runs it.  No GPU.
#include <algorithm>
#include <cstdio>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "../../ros_stereo_slam_amd/csrc/pg_solve_plan.hip.h"

using namespace pg_solve_plan;

#define EXPECT(cond)                                                                        \
    do {                                                                                    \
        if (!(cond)) {                                                                      \
            std::fprintf(stderr, "%s:%d: %s: %s\n", __FILE__, __LINE__, what.c_str(), #cond); \
            return 1;                                                                       \
        }                                                                                   \
    } while (0)

struct TestGraph {
    std::string name;
    int nv;
    std::vector<int> from, to;
};

// vertices 0 .. nv - 1, vertex 0 fixed; the odometry edge k - 1 -> k, then the closures k -> closures[.].second of vertex k, as a
// graph grows (svo_pg_augment_node, svo_pg_add_loop_closure)
static TestGraph chain(const std::string &name, int nv, const std::vector<std::pair<int, int>> &closures)
{
    TestGraph g{name, nv, {}, {}};
    for (int k = 1; k < nv; k++) {
        g.from.push_back(k - 1), g.to.push_back(k);
        for (const auto &c : closures)
            if (c.first == k)
                g.from.push_back(k), g.to.push_back(c.second);
    }
    return g;
}

// the separators the solve's LDS holds, from the constants: (2 ldr + TB) doubles in 158 KiB, ldr a multiple of TB >= 6 m
static int lds_max_separators() { return (int)((158 * 1024 / 8 - TB) / 2 / TB * TB / 6); }

static std::vector<TestGraph> graphs()
{
    std::vector<TestGraph> gs;
    gs.push_back(chain("2 vertices", 2, {}));
    for (int nb : {SEG_L - 1, SEG_L, SEG_L + 1, 2 * SEG_L + 1})
        gs.push_back(chain("chain of " + std::to_string(nb) + " unknowns", nb + 1, {}));
    gs.push_back(chain("closure to the fixed vertex", 40, {{39, 0}}));
    gs.push_back(chain("closure between neighbours", 10, {{5, 4}}));
    gs.push_back(chain("closures that share an endpoint", 50, {{48, 3}, {49, 3}}));
    gs.push_back(chain("the same closure twice", 60, {{40, 10}, {40, 10}}));
    {
        std::vector<std::pair<int, int>> c;
        for (int k = 0; k < 10; k++)
            c.push_back({250 + 2 * k, 20 + 2 * k});
        gs.push_back(chain("ten closures between two segments", 320, c));
    }
    {  // the benchmark's graph: closure k from vertex 493 + 100 k into the first lap
        std::vector<std::pair<int, int>> c;
        for (int k = 0; k < 40; k++)
            c.push_back({493 + 100 * k, 100 * (k % 5) + 8 * (k / 5)});
        gs.push_back(chain("bench", 4541, c));
    }
    {  // one closure more than the separator solve holds separators, all endpoints distinct: the cover alone is too many
        std::vector<std::pair<int, int>> c;
        const int n = lds_max_separators() + 1;
        for (int k = 0; k < n; k++)
            c.push_back({2 * n + 40 + 2 * k, 1 + 2 * k});
        gs.push_back(chain("refused", 4 * n + 80, c));
    }
    return gs;
}

static int check_plan(const std::string &what, const TestGraph &g, const Plan &p)
{
    const int nv = g.nv, nb = nv - 1, ne = (int)g.from.size(), m = p.m, nseg = p.nseg, nrb = p.nrblocks;
    const std::vector<int> &hs = p.buf;
    // the incidence lists
    EXPECT((int)p.incptr.size() == nv + 1 && p.incptr[0] == 0 && p.incptr[nv] == 2 * ne && (int)p.inc.size() == 2 * ne);
    for (int v = 0; v < nv; v++) {
        EXPECT(p.incptr[v] <= p.incptr[v + 1]);
        for (int k = p.incptr[v]; k < p.incptr[v + 1]; k++) {
            const int e = p.inc[k] >> 1, role = p.inc[k] & 1;
            EXPECT(e >= 0 && e < ne && (role ? g.to[e] : g.from[e]) == v && (k == p.incptr[v] || p.inc[k - 1] < p.inc[k]));
        }
    }
    // the layout of the buffer: every array starts where the one before it ends
    EXPECT(m >= 0 && nseg >= 0 && nrb >= 0);
    EXPECT(p.o_seg_start == 0 && p.o_seg_len == p.o_seg_start + nseg && p.o_sepidx == p.o_seg_len + nseg);
    EXPECT(p.o_lsep == p.o_sepidx + nb && p.o_rsep == p.o_lsep + nb && p.o_rowseg == p.o_rsep + nb && p.o_cptr == p.o_rowseg + nb);
    EXPECT(p.o_clrow == p.o_cptr + nseg + 1 && p.o_clrow <= hs.size());
    const int *seg_start = &hs[p.o_seg_start], *seg_len = &hs[p.o_seg_len], *sepidx = &hs[p.o_sepidx], *lsep = &hs[p.o_lsep],
              *rsep = &hs[p.o_rsep], *rowseg = &hs[p.o_rowseg], *cptr = &hs[p.o_cptr];
    const int ncl = cptr[nseg];
    EXPECT(ncl >= 0 && p.o_cedge == p.o_clrow + ncl && p.o_ctr == p.o_cedge + ncl && p.o_cwbase == p.o_ctr + ncl);
    EXPECT(p.o_csep == p.o_cwbase + ncl && p.o_rb_row == p.o_csep + ncl && p.o_rb_col == p.o_rb_row + nrb);
    EXPECT(p.o_rptr == p.o_rb_col + nrb && p.o_rptr + nrb + m + 1 <= hs.size());
    EXPECT(p.o_terms % 4 == 0 && p.o_terms >= p.o_rptr + nrb + m + 1 && p.o_terms < p.o_rptr + nrb + m + 1 + 4);
    EXPECT(p.o_rsrc >= p.o_terms && (p.o_rsrc - p.o_terms) % 4 == 0 && p.o_rsrc <= hs.size());
    const int *clrow = &hs[p.o_clrow], *cedge = &hs[p.o_cedge], *ctr = &hs[p.o_ctr], *cwbase = &hs[p.o_cwbase], *csep = &hs[p.o_csep],
              *rb_row = &hs[p.o_rb_row], *rb_col = &hs[p.o_rb_col], *rptr = &hs[p.o_rptr];
    const int nterms = (int)((p.o_rsrc - p.o_terms) / 4), nsrc = rptr[nrb + m];
    EXPECT(nsrc >= 0 && hs.size() == p.o_rsrc + 2 * (size_t)nsrc);
    const PgTerm *terms = reinterpret_cast<const PgTerm *>(hs.data() + p.o_terms);
    const Src *rsrc = reinterpret_cast<const Src *>(hs.data() + p.o_rsrc);
    static_assert(sizeof(PgTerm) == 16 && sizeof(Src) == 8, "the kernels read them as four and two ints");
    // separators and segments: a row is a separator or lies in exactly one segment
    std::vector<int> covered(nb, 0);
    int longest = 0;
    for (int sg = 0; sg < nseg; sg++) {
        const int a = seg_start[sg], l = seg_len[sg];
        EXPECT(a >= 0 && l >= 1 && l <= SEG_L && a + l <= nb && (sg == 0 || a > seg_start[sg - 1] + seg_len[sg - 1]));
        longest = std::max(longest, l);
        for (int r = a; r < a + l; r++) {
            covered[r]++;
            EXPECT(rowseg[r] == sg && sepidx[r] == -1);
            EXPECT(lsep[r] == (a > 0 ? sepidx[a - 1] : -1) && rsep[r] == (a + l < nb ? sepidx[a + l] : -1));
            EXPECT((a == 0 || lsep[r] >= 0) && (a + l == nb || rsep[r] >= 0));
        }
    }
    EXPECT(p.maxseg == longest);
    int seps = 0;
    for (int r = 0; r < nb; r++) {
        EXPECT(covered[r] == (sepidx[r] >= 0 ? 0 : 1));
        if (sepidx[r] >= 0) {
            EXPECT(sepidx[r] == seps && rowseg[r] == -1 && lsep[r] == -1 && rsep[r] == -1);
            seps++;
        }
    }
    EXPECT(seps == m);
    EXPECT(p.T == (6 * m + TB - 1) / TB && p.ldr == p.T * TB && p.ldr >= 6 * m);
    // the closures: one endpoint at least is a separator; what ends inside a segment is in its list, at most PG_MAX_SEG_CHORDS
    std::vector<int> inside(nseg, 0);
    for (int e = 0; e < ne; e++) {
        const int i = g.from[e] - 1, j = g.to[e] - 1;
        if (i < 0 || j < 0 || i == j || i - j == 1 || j - i == 1)
            continue;
        EXPECT(sepidx[i] >= 0 || sepidx[j] >= 0);
        for (int r : {i, j})
            if (sepidx[r] < 0)
                inside[rowseg[r]]++;
    }
    size_t wc = 0;
    EXPECT(cptr[0] == 0);
    for (int sg = 0; sg < nseg; sg++) {
        EXPECT(cptr[sg] <= cptr[sg + 1] && cptr[sg + 1] - cptr[sg] == inside[sg] && inside[sg] <= PG_MAX_SEG_CHORDS);
        for (int c = cptr[sg]; c < cptr[sg + 1]; c++) {
            EXPECT(clrow[c] >= 0 && clrow[c] < seg_len[sg] && cedge[c] >= 0 && cedge[c] < ne && (ctr[c] == 0 || ctr[c] == 1));
            EXPECT(csep[c] >= 0 && csep[c] < m);
            const int inner = seg_start[sg] + clrow[c] + 1, sep_v = ctr[c] ? g.from[cedge[c]] : g.to[cedge[c]];
            EXPECT((ctr[c] ? g.to[cedge[c]] : g.from[cedge[c]]) == inner && sep_v >= 1 && sepidx[sep_v - 1] == csep[c]);
            EXPECT(cwbase[c] >= 0 && (size_t)cwbase[c] == wc);  // [wbase, wbase + seg_len): one after the other, disjoint
            wc += seg_len[sg];
        }
    }
    EXPECT(wc == p.wc_blocks);
    // the gather lists
    EXPECT(rptr[0] == 0);
    std::set<std::pair<int, int>> seen;
    for (int k = 0; k < nrb + m; k++) {
        EXPECT(rptr[k] <= rptr[k + 1]);
        const bool block = k < nrb;
        if (block) {
            EXPECT(rb_row[k] >= rb_col[k] && rb_col[k] >= 0 && rb_row[k] < m && seen.insert({rb_row[k], rb_col[k]}).second);
            EXPECT(k == 0 || std::make_pair(rb_row[k - 1], rb_col[k - 1]) < std::make_pair(rb_row[k], rb_col[k]));
        }
        for (int t = rptr[k]; t < rptr[k + 1]; t++) {
            const int kind = rsrc[t].kind, idx = rsrc[t].idx;
            if (kind == SRC_DG)
                EXPECT(idx >= 0 && idx < nb && sepidx[idx] == (block ? rb_row[k] : k - nrb) && (!block || rb_row[k] == rb_col[k]));
            else if (kind == SRC_CC)
                EXPECT(block && idx >= 0 && idx < nb - 1 && sepidx[idx] == rb_col[k] && sepidx[idx + 1] == rb_row[k]);
            else if (kind == SRC_HIJ || kind == SRC_HIJ_T) {
                EXPECT(block && idx >= 0 && idx < ne);
                const int hi = (kind == SRC_HIJ ? g.from : g.to)[idx] - 1, lo = (kind == SRC_HIJ ? g.to : g.from)[idx] - 1;
                EXPECT(lo >= 0 && hi > lo && sepidx[hi] == rb_row[k] && sepidx[lo] == rb_col[k]);
            } else {
                EXPECT(kind == SRC_TERM && idx >= 0 && idx < nterms);
                const PgTerm &tm = terms[idx];
                if (tm.a_kind == A_CC || tm.a_kind == A_CC_T)
                    EXPECT(tm.a >= 0 && tm.a < nb - 1);
                else
                    EXPECT((tm.a_kind == A_HIJ || tm.a_kind == A_HIJ_T) && tm.a >= 0 && tm.a < ne);
                if (block) {
                    if (tm.w_kind == W_L || tm.w_kind == W_R)
                        EXPECT(tm.w >= 0 && tm.w < nb && sepidx[tm.w] < 0);
                    else
                        EXPECT(tm.w_kind == W_C && tm.w >= 0 && (size_t)tm.w < p.wc_blocks);
                } else
                    EXPECT(tm.w_kind == W_Y && tm.w >= 0 && tm.w < nb && sepidx[tm.w] < 0);
            }
        }
    }
    for (int k = 0; k < m; k++)  // every separator has its diagonal block and its right-hand side
        EXPECT(seen.count({k, k}) && rptr[nrb + k] < rptr[nrb + k + 1]);
    return 0;
}

int main()
{
    const int bound = (158 * 1024 / 16 - TB) / 6;  // the number the refusal names
    for (const TestGraph &g : graphs()) {
        Plan plans[3];
        for (int force : {0, 1, -1}) {
            Plan &p = plans[force < 0 ? 2 : force];
            const std::string what = g.name + ", force " + std::to_string(force);
            build(g.nv, (int)g.from.size(), g.from.data(), g.to.data(), force, p);
            if (check_plan(what, g, p))
                return 1;
            EXPECT(solve_lds_refusal(p) == (g.name == "refused" ? bound : 0));
            if (g.name == "refused")
                EXPECT(p.m > lds_max_separators() && (size_t)(2 * p.ldr + TB) * 8 > 158 * 1024);
            else
                EXPECT(p.m <= lds_max_separators());
        }
        const std::string what = g.name;
        const Plan &both = plans[0], &cover = plans[1], &model = plans[2];
        EXPECT(model.buf == both.buf || model.buf == cover.buf);
        EXPECT(cover.m <= both.m);
        const int nb = g.nv - 1;
        if (g.from.size() == (size_t)nb) {  // a chain: no closure, one structure; a regular separator where a run reaches SEG_L rows,
                                            // but not on the last row
            EXPECT(both.buf == cover.buf && both.m == (nb - 1) / SEG_L && both.maxseg == std::min(nb, both.m ? SEG_L - 1 : SEG_L));
            EXPECT(both.nseg == both.m + 1 && both.wc_blocks == 0 && both.nrblocks == (both.m ? 2 * both.m - 1 : 0));
        }
        if (g.name == "closure to the fixed vertex" || g.name == "closure between neighbours")  // no chord
            EXPECT(both.m == 0 && cover.m == 0 && both.nseg == 1 && both.buf == cover.buf);
        if (g.name == "closures that share an endpoint")  // rows 2, 47, 48; the cover: 47 and 48 (the later row of each)
            EXPECT(both.m == 3 && both.wc_blocks == 0 && cover.m == 2 && cover.wc_blocks == 2 * 47);
        if (g.name == "the same closure twice")  // rows 9 and 39; the cover: 39, and both edges end inside the first segment
            EXPECT(both.m == 2 && both.nrblocks == 3 && cover.m == 1 && cover.wc_blocks == 2 * 39);
        if (g.name == "ten closures between two segments")
            // the cover takes the ten later rows; the ten earlier ones lie in one segment, which holds eight: two more separators
            // (and the regular ones at rows 141 and 245 of the run between the two groups)
            EXPECT(both.m == 20 + 2 && cover.m == 10 + 2 + 2 && cover.wc_blocks == 8 * 35);
        if (g.name == "bench")
            // pg_solve_plan.hip.h's comment on the two structures: the cover's 45 separators and 5 tile steps against both ends' 9, and
            // the model takes both ends.  Both ends are 80 separators here, not the comment's 81: this graph's first closure ends on
            // the fixed vertex and is no chord (39 chords, 78 endpoints, 2 regular separators).
            EXPECT(cover.m == 45 && cover.T == 6 && both.m == 80 && both.T == 10 && model.buf == both.buf);
    }
    std::puts("pg solve plan check ok");
    return 0;
}
