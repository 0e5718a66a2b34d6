// pg_solve_plan.hip.h -- the elimination structure of the pose graph's linear solve with nothing of HIP in it: the incidence lists,
// the separators (both ends of every closure, or a cover of them, by a small cost model), the segments between them, what couples a
// segment to the separators, the gather lists of the reduced system and the one int buffer the kernels read all of it from -- every
// index a kernel of posegraph.hip follows is computed here.  Also the constants, the kinds of a gather's sources and terms (host and
// pg_reduce_kernel use the same names) and the bound of the separator solve's LDS.  posegraph.hip includes it; so does
// tests/cpp/pg_solve_plan_check.cpp, a stand-alone program that runs it under the address and undefined-behaviour sanitizers.
#pragma once

#include <cstddef>
#include <map>
#include <vector>

namespace pg_solve_plan {

constexpr int PG_MAX_SEG_CHORDS = 8;  // closure endpoints a segment takes inside (six right-hand-side columns each, two to a pass)
constexpr int SEG_L = 104;  // regular separator spacing (rows): a segment and its 13 right-hand sides live in LDS
constexpr int TB = 48;      // tile of the dense reduced solve (8 block rows)

// One source of a gather list of the reduced system, (kind, idx): what pg_reduce_kernel adds to a 6 x 6 block or to a right-hand side.
struct Src {  // the kernel reads it as an int2
    int kind, idx;
};
enum SrcKind : int {
    SRC_DG = 0,     // + Dg[idx]  (right-hand side: + rneg[idx])
    SRC_CC = 1,     // + Cc[idx]
    SRC_HIJ = 2,    // + Hij of edge idx
    SRC_HIJ_T = 3,  // + Hij^T of edge idx
    SRC_TERM = 7,   // - A^T W, term idx of the table
};
// A term: a segment couples to separator u through the block A = H[row_u][u] and to separator v through
// W_v = T^-1 E_{row_v} H[row_v][v]; the Schur complement takes A^T W_v[row_u] off the block (u, v) -- and A^T Y[row_u] off u's
// right-hand side.
enum AKind : int {
    A_CC = 0,     // Cc[a] (the segment's first row and the separator before it)
    A_CC_T = 1,   // Cc[a]^T (its last row and the separator after it)
    A_HIJ = 2,    // a closure's Hij (an endpoint inside the segment and the one that is a separator)
    A_HIJ_T = 3,  // ... Hij^T
};
static_assert(A_CC < A_HIJ && A_CC_T < A_HIJ && (A_CC_T & 1) && (A_HIJ_T & 1) && !(A_CC & 1) && !(A_HIJ & 1),
              "pg_reduce_kernel: kinds below A_HIJ read Cc, the odd ones are the transposes");
enum WKind : int { W_L = 0, W_R = 1, W_C = 2, W_Y = 3 };  // Wl, Wr, Wc (6 x 6 block w), Y (6-vector w)
struct PgTerm {
    int a_kind, a, w_kind, w;
};

struct Plan {
    // incident edges of vertex v: inc[incptr[v] .. incptr[v + 1]) = edge * 2 + role (0: v is the edge's `from`, 1: `to`), ascending
    std::vector<int> incptr, inc;
    // every other array, one after the other; o_*: where each starts (in ints)
    std::vector<int> buf;
    size_t o_seg_start = 0, o_seg_len = 0;                          // [nseg] a segment's first row and its rows
    size_t o_sepidx = 0, o_lsep = 0, o_rsep = 0, o_rowseg = 0;      // [nb] a row's separator index or -1; the separators left and
                                                                    // right of its segment or -1; its segment or -1
    size_t o_cptr = 0;                                              // [nseg + 1] the closures that end inside a segment:
    size_t o_clrow = 0, o_cedge = 0, o_ctr = 0, o_cwbase = 0, o_csep = 0;  // row within it, edge, Hij^T?, first Wc block, separator
    size_t o_rb_row = 0, o_rb_col = 0;                              // [nrblocks] the reduced system's blocks, row >= col
    size_t o_rptr = 0;                                              // [nrblocks + m + 1] sources of a block / of a right-hand side
    size_t o_terms = 0;                                             // PgTerm each; a multiple of four ints
    size_t o_rsrc = 0;                                              // Src each
    int m = 0, nseg = 0, nrblocks = 0;                              // separators, segments, blocks
    int T = 0, ldr = 0;                                             // tiles of the reduced system and its leading dimension T * TB
    int maxseg = 0;                                                 // rows of the longest segment
    size_t wc_blocks = 0;                                           // 6 x 6 blocks of Wc
};

// chords: the edges between non-neighbouring unknowns (loop closures)
struct Chord {
    int e, i, j;  // rows of `from` and `to`
};

struct Separators {
    std::vector<char> is_sep;
    std::vector<int> sepidx, seps, seg_start, seg_len, lsep, rsep, rowseg;
};

// The separators of one structure (both_ends or the cover, below) and the segments between them -> the closure endpoints inside
// the fullest segment.  A regular separator goes where a run would reach SEG_L rows, but not onto the last row: a tail segment has
// up to SEG_L rows, the others SEG_L - 1.
inline int select_separators(const int nb, const std::vector<Chord> &chords, const bool both_ends, Separators &s)
{
    std::vector<char> cover(nb, 0);
    for (const Chord &c : chords) {
        if (both_ends)
            cover[c.i] = cover[c.j] = 1;
        else if (!cover[c.i] && !cover[c.j])
            cover[c.i > c.j ? c.i : c.j] = 1;
    }
    int fullest = 0;
    for (;;) {
        s.is_sep = cover;
        for (int b = 0, run = 0; b < nb - 1; b++) {
            if (s.is_sep[b]) {
                run = 0;
                continue;
            }
            if (++run >= SEG_L) {
                s.is_sep[b] = 1;
                run = 0;
            }
        }
        s.sepidx.assign(nb, -1);
        s.seps.clear();
        for (int b = 0; b < nb; b++)
            if (s.is_sep[b]) {
                s.sepidx[b] = (int)s.seps.size();
                s.seps.push_back(b);
            }
        s.seg_start.clear();
        s.seg_len.clear();
        s.lsep.assign(nb, -1);
        s.rsep.assign(nb, -1);
        s.rowseg.assign(nb, -1);
        for (int b = 0; b < nb;) {
            if (s.is_sep[b]) {
                b++;
                continue;
            }
            int z = b;
            while (z + 1 < nb && !s.is_sep[z + 1])
                z++;
            for (int r = b; r <= z; r++) {
                s.lsep[r] = b > 0 ? s.sepidx[b - 1] : -1;
                s.rsep[r] = z + 1 < nb ? s.sepidx[z + 1] : -1;
                s.rowseg[r] = (int)s.seg_start.size();
            }
            s.seg_start.push_back(b);
            s.seg_len.push_back(z - b + 1);
            b = z + 1;
        }
        // a segment with too many closure endpoints inside: the surplus becomes separators, and once more
        std::vector<int> inside(s.seg_start.size(), 0);
        bool again = false;
        fullest = 0;
        for (const Chord &c : chords)
            for (const int r : {c.i, c.j})
                if (!s.is_sep[r]) {
                    if (++inside[s.rowseg[r]] > PG_MAX_SEG_CHORDS) {
                        cover[r] = 1;
                        again = true;
                    } else if (inside[s.rowseg[r]] > fullest)
                        fullest = inside[s.rowseg[r]];
                }
        if (!again)
            break;
    }
    return fullest;
}

// What a solve with n_seps separators and `fullest` closure endpoints inside its fullest segment costs beyond what both
// structures share, in microseconds (measured constants): a tile step of the dense factorisation, a tile of the separator solve, a
// pass of six more right-hand-side columns (two closures to a pass) through the segments.
inline double cost_us(const int n_seps, const int fullest)
{
    const int tiles = (6 * n_seps + TB - 1) / TB;
    return 16.7 * (tiles > 1 ? tiles - 1 : 0) + 2.3 * tiles + 23.0 * ((fullest + 1) / 2);
}

// The structure of a graph of nv vertices (vertex 0 is fixed: unknown block b = vertex b + 1, nb = nv - 1 >= 1) and ne >= 1 edges.
// force: -1 the cheaper structure by the cost model, 0 both ends, 1 the cover.  The order of everything in `buf` -- the arrays, the
// blocks (row, then column), the sources within a block -- is the order of the kernels' sums: a change changes the bits of a solve.
inline void build(const int nv, const int ne, const int *efrom, const int *eto, const int force, Plan &plan)
{
    const int nb = nv - 1;
    std::vector<int> &incptr = plan.incptr, &inc = plan.inc, &hs = plan.buf;
    incptr.assign(nv + 1, 0);
    inc.assign(2 * (size_t)ne, 0);
    for (int e = 0; e < ne; e++) {
        incptr[efrom[e] + 1]++;
        incptr[eto[e] + 1]++;
    }
    for (int v = 0; v < nv; v++)
        incptr[v + 1] += incptr[v];
    {
        std::vector<int> fill(incptr.begin(), incptr.end() - 1);
        for (int e = 0; e < ne; e++) {  // ascending edge index within each vertex
            inc[fill[efrom[e]]++] = 2 * e;
            inc[fill[eto[e]]++] = 2 * e + 1;
        }
    }
    std::vector<Chord> chords;
    for (int e = 0; e < ne; e++) {
        const int i = efrom[e] - 1, j = eto[e] - 1;
        if (i < 0 || j < 0 || i == j || i - j == 1 || j - i == 1)
            continue;
        chords.push_back({e, i, j});
    }
    // Separators: every separator adds six rows to the dense reduced system, whose tile steps are what a solve's time is
    // made of.  Two structures, the cheaper by a small cost model (measured constants) is taken:
    //   both   BOTH endpoints of every chord + a regular one only where that leaves a run longer than SEG_L - 1 rows;
    //   cover  a COVER of the chords (where neither endpoint of a chord is a separator yet, the later row becomes one);
    //          a chord's other endpoint stays inside its segment and costs that segment a pass of six more right-hand-
    //          side columns (pg_segment_kernel: two closures to a pass, at most PG_MAX_SEG_CHORDS per segment, the
    //          ones beyond that become separators after all).
    // At 4541 vertices / 40 closures whose matches all lie in the first lap: cover = 45 separators instead of 81 (5 tile
    // steps instead of 9, the solve 12 us instead of 25: -80 us) but four passes of 23 us in each of the first lap's
    // segments (+91 us): 0.292 against 0.279 ms per iteration, and the model says so; closures whose endpoints spread
    // take one pass per segment and the cover.  SVO_PG_COVER=1 / 0 forces one or the other (the tests run both).
    Separators s;
    {
        bool both_ends = force == 0;
        if (force < 0) {
            const int fullest_both = select_separators(nb, chords, true, s);
            const double both = cost_us((int)s.seps.size(), fullest_both);
            const int fullest_cover = select_separators(nb, chords, false, s);
            both_ends = both <= cost_us((int)s.seps.size(), fullest_cover);
        }
        (void)select_separators(nb, chords, both_ends, s);
    }
    const std::vector<char> &is_sep = s.is_sep;
    const std::vector<int> &sepidx = s.sepidx, &seps = s.seps, &seg_start = s.seg_start, &seg_len = s.seg_len, &rowseg = s.rowseg;
    const int m = (int)seps.size(), n_seg = (int)seg_start.size();
    // what couples a segment to the separators: its two neighbours in the chain, and the closures that end inside it
    struct Coupling {
        int row, sep, a_kind, a, w_kind, wbase;  // W block of row r: Wl / Wr: r itself; Wc: wbase + (r - segment start)
    };
    std::vector<std::vector<Coupling>> coup(n_seg);
    std::vector<int> cptr(n_seg + 1, 0), c_lrow, c_edge, c_tr, c_wbase, c_sep;
    for (int sg = 0; sg < n_seg; sg++) {
        const int a = seg_start[sg], z = a + seg_len[sg] - 1;
        if (a > 0)
            coup[sg].push_back({a, sepidx[a - 1], A_CC, a - 1, W_L, 0});
        if (z < nb - 1)
            coup[sg].push_back({z, sepidx[z + 1], A_CC_T, z, W_R, 0});
    }
    size_t wc_blocks = 0;
    {
        std::vector<std::vector<Coupling>> inner(n_seg);
        for (const Chord &c : chords) {
            if (is_sep[c.i] && is_sep[c.j])
                continue;
            // (the cover: at least one endpoint is a separator)
            const bool from_inside = !is_sep[c.i];
            const int r = from_inside ? c.i : c.j, sp = from_inside ? c.j : c.i, sg = rowseg[r];
            // H[r][sp]: r = `from`: Hij; r = `to`: Hij^T
            inner[sg].push_back({r, sepidx[sp], from_inside ? A_HIJ : A_HIJ_T, c.e, W_C, 0});
        }
        for (int sg = 0; sg < n_seg; sg++) {
            for (Coupling &k : inner[sg]) {
                k.wbase = (int)wc_blocks;
                wc_blocks += seg_len[sg];
                c_lrow.push_back(k.row - seg_start[sg]);
                c_edge.push_back(k.a);
                c_tr.push_back(k.a_kind == A_HIJ_T ? 1 : 0);
                c_wbase.push_back(k.wbase);
                c_sep.push_back(k.sep);
                coup[sg].push_back(k);
            }
            cptr[sg + 1] = (int)c_lrow.size();
        }
    }
    // gather lists of the reduced system
    struct Key {
        int r, c;
        bool operator<(const Key &o) const { return r != o.r ? r < o.r : c < o.c; }
    };
    std::map<Key, std::vector<Src>> blocks;
    std::vector<std::vector<Src>> rhs_src(m);
    std::vector<int> terms;  // PgTerm: a_kind, a, w_kind, w
    auto term = [&](const Coupling &u, int w_kind, int w) {
        terms.insert(terms.end(), {u.a_kind, u.a, w_kind, w});
        return Src{SRC_TERM, (int)(terms.size() / 4 - 1)};
    };
    for (int k = 0; k < m; k++) {
        const int sr = seps[k];
        blocks[{k, k}].push_back({SRC_DG, sr});
        rhs_src[k].push_back({SRC_DG, sr});
        if (k > 0 && seps[k - 1] + 1 == sr)
            blocks[{k, k - 1}].push_back({SRC_CC, seps[k - 1]});
    }
    for (const Chord &c : chords)
        if (is_sep[c.i] && is_sep[c.j]) {  // block(row i, col j) = Ji^T Jj; stored at (hi, lo)
            if (c.i > c.j)
                blocks[{sepidx[c.i], sepidx[c.j]}].push_back({SRC_HIJ, c.e});
            else
                blocks[{sepidx[c.j], sepidx[c.i]}].push_back({SRC_HIJ_T, c.e});
        }
    for (int sg = 0; sg < n_seg; sg++)
        for (const Coupling &u : coup[sg]) {
            rhs_src[u.sep].push_back(term(u, W_Y, u.row));
            for (const Coupling &v : coup[sg]) {
                if (u.sep < v.sep)
                    continue;  // the lower triangle; for u.sep == v.sep both orders are terms of the diagonal block
                const int w = v.w_kind == W_C ? v.wbase + (u.row - seg_start[sg]) : u.row;
                blocks[{u.sep, v.sep}].push_back(term(u, v.w_kind, w));
            }
        }
    std::vector<int> rb_row, rb_col, rptr(1, 0);
    std::vector<Src> rsrc;
    for (auto &kv : blocks) {
        rb_row.push_back(kv.first.r);
        rb_col.push_back(kv.first.c);
        rsrc.insert(rsrc.end(), kv.second.begin(), kv.second.end());
        rptr.push_back((int)rsrc.size());
    }
    for (int k = 0; k < m; k++) {  // right-hand sides
        rsrc.insert(rsrc.end(), rhs_src[k].begin(), rhs_src[k].end());
        rptr.push_back((int)rsrc.size());
    }
    plan.m = m;
    plan.nseg = n_seg;
    plan.maxseg = 0;
    for (int l : seg_len)
        plan.maxseg = l > plan.maxseg ? l : plan.maxseg;
    plan.nrblocks = (int)blocks.size();
    plan.T = (6 * m + TB - 1) / TB;
    plan.ldr = plan.T * TB;
    plan.wc_blocks = wc_blocks;
    // one int buffer for all the structure arrays
    hs.clear();
    auto put = [&](const std::vector<int> &v) {
        const size_t off = hs.size();
        hs.insert(hs.end(), v.begin(), v.end());
        return off;
    };
    plan.o_seg_start = put(seg_start);
    plan.o_seg_len = put(seg_len);
    plan.o_sepidx = put(sepidx);
    plan.o_lsep = put(s.lsep);
    plan.o_rsep = put(s.rsep);
    plan.o_rowseg = put(rowseg);
    plan.o_cptr = put(cptr);
    plan.o_clrow = put(c_lrow);
    plan.o_cedge = put(c_edge);
    plan.o_ctr = put(c_tr);
    plan.o_cwbase = put(c_wbase);
    plan.o_csep = put(c_sep);
    plan.o_rb_row = put(rb_row);
    plan.o_rb_col = put(rb_col);
    plan.o_rptr = put(rptr);
    while (hs.size() & 3)
        hs.push_back(0);
    plan.o_terms = put(terms);
    plan.o_rsrc = hs.size();
    for (const Src &v : rsrc) {
        hs.push_back(v.kind);
        hs.push_back(v.idx);
    }
}

// The separator solve keeps its vector and its running sums in one workgroup's LDS, (2 ldr + TB) doubles of the 158 KiB it may
// take.  0 when the plan's solve fits; else the number of separators the refusal names.
inline int solve_lds_refusal(const Plan &plan)
{
    constexpr size_t LDS_MAX = 158 * 1024;
    return (size_t)(2 * plan.ldr + TB) * 8 > LDS_MAX ? (int)((LDS_MAX / 16 - TB) / 6) : 0;
}

}  // namespace pg_solve_plan
