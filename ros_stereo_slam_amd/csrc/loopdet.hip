// loopdet.hip -- the loop-closure detector on gfx950.
//
// Replaces visualSLAM::checkLoopDetectorStatus (src/optimizationStuff.cpp:49-64): features by
// orb.hip, then DLoopDetector::detectLoop (include/TemplatedLoopDetector.h:696-861) with the
// parameters visualSLAM sets (include/visualSLAM.h:120-127) on top of Parameters::set(1)
// (:552-568).  The control flow -- database query below `dislocal`, normalisation by the score
// against the previous frame, alpha cut, islands (:875-951), temporal window (:966-1003), geometric
// check by neighbour-ratio matches + a RANSAC fundamental matrix (:1101-1160, :1255-1316) -- follows
// the vendored header; it is host code, a few dozen integers per frame.
//
// Stated deviation (also oracle/loopdet.c): DBoW2, DLib and the vocabulary orb_voc00.yml.gz were
// stripped from the reference checkout, so the bag-of-words score is replaced by a vocabulary-free
// similarity on the same 256-bit descriptors -- the fraction of query descriptors with a neighbour
// within a Hamming radius in the entry -- and GEOM_DI's direct index by the header's own exhaustive
// neighbour-ratio matching.  The data-parallel part is that similarity: every database entry
// against the query = N_db x 500 x 500 Hamming distances per frame (popcounts of XORs, entry
// descriptors staged in LDS and read as broadcasts), one workgroup per entry.
#include <algorithm>
#include <deque>
#include <vector>

#include "svo_internal.h"
#include "wave_ops.hip.h"

namespace {

__device__ __forceinline__ int hamming256(const uint32_t (&a)[8], const uint32_t *b)
{
    int d = 0;
#pragma unroll
    for (int k = 0; k < 8; k++)
        d += __popc(a[k] ^ b[k]);
    return d;
}

// counts[e] = number of query descriptors whose nearest descriptor of entry e is within thr
__global__ __launch_bounds__(256) void lc_score_kernel(const uint32_t *__restrict__ q, const int *__restrict__ d_nq,
                                                       const uint32_t *__restrict__ db, const int *__restrict__ db_n,
                                                       int stride, int thr, int *__restrict__ counts)
{
    extern __shared__ uint32_t s_e[];  // stride * 8 words
    __shared__ int s_red[4];
    const int e = blockIdx.x, t = threadIdx.x;
    const int ne = db_n[e], nq = *d_nq;
    const uint32_t *E = db + (size_t)e * stride * 8;
    for (int i = t; i < ne * 8; i += 256)
        s_e[i] = E[i];
    __syncthreads();
    int c = 0;
    for (int i = t; i < nq; i += 256) {
        uint32_t a[8];
#pragma unroll
        for (int k = 0; k < 8; k++)
            a[k] = q[(size_t)8 * i + k];
        int best = 1 << 30;
        for (int j = 0; j < ne; j++) {
            const int d = hamming256(a, s_e + 8 * j);
            best = d < best ? d : best;
        }
        c += best <= thr ? 1 : 0;
    }
    c = svo::wave_sum(c);
    if ((t & 63) == 0)
        s_red[t >> 6] = c;
    __syncthreads();
    if (t == 0)
        counts[e] = s_red[0] + s_red[1] + s_red[2] + s_red[3];
}

// getMatches_neighratio's search (:1268-1291): nearest B (first on ties), its distance, the second best
__global__ __launch_bounds__(256) void lc_nearest2_kernel(const uint32_t *__restrict__ A, int na,
                                                          const uint32_t *__restrict__ B, const int *__restrict__ d_nb,
                                                          int *__restrict__ best_j, int *__restrict__ d1,
                                                          int *__restrict__ d2)
{
    extern __shared__ uint32_t s_b[];
    const int nb = *d_nb;
    for (int i = threadIdx.x; i < nb * 8; i += 256)
        s_b[i] = B[i];
    __syncthreads();
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= na)
        return;
    uint32_t a[8];
#pragma unroll
    for (int k = 0; k < 8; k++)
        a[k] = A[(size_t)8 * i + k];
    int bj = -1, b1 = 1000000000, b2 = 1000000000;
    for (int j = 0; j < nb; j++) {
        const int d = hamming256(a, s_b + 8 * j);
        if (d < b1) {
            bj = j;
            b2 = b1;
            b1 = d;
        } else if (d < b2)
            b2 = d;
    }
    best_j[i] = bj;
    d1[i] = b1;
    d2[i] = b2;
}

// What the host logic of one frame needs, reduced on the device and left in pinned memory: the number of query
// features, the similarity count against the previous entry (the normalisation score, :736-739) and the
// max_db_results best entries below `dislocal` -- count descending, entry id ascending on ties, what
// std::stable_sort + resize of the full result list gives (:714-722) -- instead of every entry's count.
constexpr int LC_MAX_CAND = 64;
struct LcRecord {
    int ready;       // entry id + 1 once the record is complete (released at system scope)
    int nq;          // query descriptors
    int last_count;  // count against entry id - 1
    int n_cand;
    int cand_id[LC_MAX_CAND], cand_count[LC_MAX_CAND];
};

__global__ __launch_bounds__(256) void lc_topk_kernel(const int *__restrict__ counts, int max_id, int k_want,
                                                      const int *__restrict__ d_nq, int entry_id, int nf, LcRecord *rec)
{
    __shared__ int s_hist[2049], s_cut, s_above, s_n, s_wave[4], s_run;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    for (int i = t; i <= nf; i += 256)
        s_hist[i] = 0;
    if (t == 0) {
        s_n = 0;
        s_run = 0;
    }
    __syncthreads();
    for (int e = t; e < max_id; e += 256) {
        const int c = min(counts[e], nf);
        if (c > 0)
            atomicAdd(&s_hist[c], 1);
    }
    __syncthreads();
    if (t == 0) {  // the count value at which the k_want-th best entry sits
        int cum = 0, cut = 1;
        for (int c = nf; c >= 1; c--) {
            if (cum + s_hist[c] >= k_want) {
                cut = c;
                break;
            }
            cum += s_hist[c];
        }
        // entries with a count above `cut` all take part (`above` of them); of those AT the cut the lowest ids fill up
        int above = 0;
        for (int c = nf; c > cut; c--)
            above += s_hist[c];
        s_cut = cut;
        s_above = above;
    }
    __syncthreads();
    const int cut = s_cut, need = max(0, min(k_want, LC_MAX_CAND) - s_above);
    for (int base = 0; base < max_id; base += 256) {
        const int e = base + t;
        const int c = e < max_id ? min(counts[e], nf) : 0;
        if (c > cut) {
            const int slot = atomicAdd(&s_n, 1);
            if (slot < LC_MAX_CAND) {
                rec->cand_id[slot] = e;
                rec->cand_count[slot] = c;
            }
        }
        // ties at the cut, in entry order
        const bool tie = c == cut && c > 0;
        const unsigned long long bal = __ballot(tie);
        if (lane == 0)
            s_wave[wave] = __popcll(bal);
        __syncthreads();
        int before = s_run;
        for (int w2 = 0; w2 < wave; w2++)
            before += s_wave[w2];
        const int pos = before + __popcll(bal & ((1ull << lane) - 1ull));
        if (tie && pos < need) {
            const int slot = atomicAdd(&s_n, 1);
            if (slot < LC_MAX_CAND) {
                rec->cand_id[slot] = e;
                rec->cand_count[slot] = c;
            }
        }
        __syncthreads();
        if (t == 0)
            s_run += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
        __syncthreads();
    }
    if (t == 0) {
        rec->nq = *d_nq;
        rec->last_count = entry_id > 0 ? counts[entry_id - 1] : 0;
        rec->n_cand = min(s_n, LC_MAX_CAND);
        __threadfence_system();
        __hip_atomic_store(&rec->ready, entry_id + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

__global__ void lc_store_int_kernel(int *dst, int v) { *dst = v; }

// The neighbour-ratio matches of the geometric checks of a look-ahead group ON THE DEVICE (getMatches_neighratio,
// include/TemplatedLoopDetector.h:1255-1316, per direct-index node :1005-1087 / over the whole image :1101-1160): one
// workgroup per check turns [best_j | d1 | d2] of the old image's features into the pair list the F-matrix RANSAC takes,
// in the order the sequential loop produces it.  That loop visits the old features by (node, index), keeps a feature whose
// d1 / d2 passes the ratio, and lets the features of one node that share their nearest current feature fight it out: the
// pair STAYS where the first of them put it, the old index becomes the one with the smallest d1 (the earliest among equals:
// only a strictly smaller distance replaces).  So: a pair per (node, best_j) key, at the rank of the key's first feature in
// (node, index) order, holding the key's (d1, index)-minimal feature -- every part a count over <= nf features.
// Round 5 did this on the host (20 ms of a 1 600-frame run's 49, between two waits per group).
struct LcGeoBatch {
    int old_entry[SVO_LK_MAX_JOBS], cur_entry[SVO_LK_MAX_JOBS], na[SVO_LK_MAX_JOBS];
};
// tail of a check's device slot (the last 256 bytes): F 9 doubles | inlier count | iterations | pairs | gate
constexpr int GEO_TAIL_PAIRS = 20, GEO_TAIL_GATE = 21, GEO_TAIL_WORDS = 22;
__global__ __launch_bounds__(512) void lc_geo_match_kernel(LcGeoBatch b, int nf, uint8_t *__restrict__ geo_dev, size_t dev_stride,
                                                           const int *__restrict__ db_node, const float *__restrict__ db_xy,
                                                           uint8_t *__restrict__ geo_up, size_t up_stride, double max_ratio, int min_pairs)
{
    // A key (node, best_j) IS its best_j: a current feature lies under one node, and the matching only pairs features of one
    // node (without a vocabulary there is one node).  So every current feature j owns a slot: the features that pass the
    // ratio drop (d1, index) and their index into the slot of their best_j with two LDS atomic minima -- the pair's old
    // feature and the feature that opened the key -- and the pairs are the slots that were hit, ranked by (node, opener).
    // (A thread per feature walking all the others took 115 us per group of checks, a wavefront per feature 196.)
    extern __shared__ int s_mem[];
    int *s_node = s_mem, *s_min = s_node + nf, *s_fst = s_min + nf;
    int *k_node = s_fst + nf, *k_fst = k_node + nf, *k_win = k_fst + nf, *k_j = k_win + nf;
    __shared__ int s_m, s_wcnt[8];
    const int s = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6, na = b.na[s];
    const int *nn = reinterpret_cast<const int *>(geo_dev + dev_stride * s);
    const size_t o = (size_t)b.old_entry[s] * nf, q = (size_t)b.cur_entry[s] * nf;
    constexpr int NONE = 0x7fffffff;
    for (int j = t; j < nf; j += 512) {
        s_min[j] = NONE;
        s_fst[j] = NONE;
    }
    if (t == 0)
        s_m = 0;
    __syncthreads();
    for (int i = t; i < na; i += 512) {
        const int node = db_node ? db_node[o + i] : 0, bj = nn[i], d1 = nn[nf + i], d2 = nn[2 * nf + i];
        s_node[i] = node;
        const bool visited = !db_node || (node >= 0 && bj >= 0);
        if (visited && (double)d1 / (double)d2 <= max_ratio && bj >= 0 && bj < nf) {   // :1293 (a Hamming distance: d1 <= 256)
            atomicMin(&s_min[bj], d1 * 4096 + i);   // the smallest d1, the earliest among equals (nf < 4096)
            atomicMin(&s_fst[bj], i);
        }
    }
    __syncthreads();
    for (int base = 0; base < nf; base += 512) {   // the slots that were hit, listed (any order: they are ranked below)
        const int j = base + t;
        const bool hit = j < nf && s_fst[j] != NONE;
        const unsigned long long bal = __ballot(hit);
        if (lane == 0)
            s_wcnt[wave] = __popcll(bal);
        __syncthreads();
        int at = s_m + __popcll(bal & ((1ull << lane) - 1ull));
        for (int w = 0; w < wave; w++)
            at += s_wcnt[w];
        if (hit) {
            const int f = s_fst[j];
            k_fst[at] = f;
            k_node[at] = s_node[f];
            k_win[at] = s_min[j] & 4095;
            k_j[at] = j;
        }
        __syncthreads();
        if (t == 0) {
            int add = 0;
            for (int w = 0; w < 8; w++)
                add += s_wcnt[w];
            s_m += add;
        }
        __syncthreads();
    }
    const int m = s_m;
    float *p1 = reinterpret_cast<float *>(geo_up + up_stride * s), *p2 = p1 + 2 * nf;
    for (int a = t; a < m; a += 512) {
        const int node = k_node[a], f = k_fst[a];
        int rank = 0;   // the keys opened before this one: the loop visits the old features by (node, index)
        for (int c = 0; c < m; c++)
            rank += (k_node[c] < node || (k_node[c] == node && k_fst[c] < f)) ? 1 : 0;
        const int A = k_win[a], B = k_j[a];
        p1[2 * rank] = db_xy[2 * (o + A)];
        p1[2 * rank + 1] = db_xy[2 * (o + A) + 1];
        p2[2 * rank] = db_xy[2 * (q + B)];
        p2[2 * rank + 1] = db_xy[2 * (q + B) + 1];
    }
    if (t == 0) {
        int *tail = reinterpret_cast<int *>(geo_dev + dev_stride * s + dev_stride - 256);
        tail[18] = 0;                               // inlier count: what a RANSAC that is not due leaves
        tail[19] = 0;
        tail[GEO_TAIL_PAIRS] = m;
        tail[GEO_TAIL_GATE] = m >= min_pairs ? 1 : 0;
    }
}

// the F-matrix, inlier count, iteration count and pair count of every check (the last 256 bytes of a slot): 22 dwords per check
__global__ void lc_geo_result_kernel(int n, const uint8_t *__restrict__ geo_dev, size_t dev_stride, uint8_t *__restrict__ host,
                                     size_t host_stride)
{
    for (int t = threadIdx.x; t < n * 32; t += blockDim.x) {
        const int s = t >> 5, w = t & 31;
        if (w < GEO_TAIL_WORDS)
            reinterpret_cast<unsigned *>(host + host_stride * s + host_stride - 256)[w] =
                reinterpret_cast<const unsigned *>(geo_dev + dev_stride * s + dev_stride - 256)[w];
    }
}

struct Island {  // tIsland, :268-330
    int first, last;
    double score;
    int best_entry;
    double best_score;
};
struct Result {
    int id;
    double score;
};

}  // namespace

constexpr int LC_BATCH = 16;   // frames per svo_lc_submit_batch group (<= dislocal: see lc_enqueue)

struct svo_lc {
    svo_ctx *ctx = nullptr;
    svo_lc_params prm;
    svo_orb *orb = nullptr;        // orb_shape 0: three factor-2 octaves (orb.hip)
    svo_orb_cv *orb_cv = nullptr;  // orb_shape 1: cv::ORB's own shape (orb_cv.hip), LC_BATCH images per launch
    int w = 0, h = 0, c = 0, nf = 0, capacity = 0;
    DevBuf db_desc, db_xy, db_n, q, counts, nn, img;
    std::vector<int> n_host;                 // descriptors per COLLECTED entry
    LcRecord *rec = nullptr;                 // pinned: one record per entry, filled by lc_topk_kernel
    int submitted = 0;                       // entries queued (svo_lc_submit); n_host.size() of them are collected
    int window_n = 0, window_first = 0, window_last = 0, window_query = -1;
    bool have_last = false;                  // m_last_bowvec's stand-in: the previous entry is the reference
    // bag-of-words mode (svo_lc_set_vocabulary): DBoW2's database.  Row e of bw_w / bw_v is entry e's BowVector (ascending
    // words, nf slots), bw_node its direct index (node per feature, -1: not indexed); the inverted file is a linked list per
    // word THROUGH the rows (bw_head per word, bw_next per row slot); bw_plane / bw_sums are the query's workspace
    svo_voc *voc = nullptr;
    int di_levels = 2;
    DevBuf bw_w, bw_v, bw_nw, bw_node, bw_head, bw_next, bw_plane, bw_sums, bw_mask, q_word, q_weight, q_node;
    svo_lc_bow_record *rec_bow = nullptr;    // pinned: one record per entry, filled by bow_topk_kernel
    uint8_t *stage = nullptr;                // pinned ring for svo_lc_submit_features with host arrays
    std::vector<hipEvent_t> stage_ev;
    long stage_next = 0;
    // the same for groups of frames (svo_lc_submit_features_batch / _fill_ with host arrays): GROUP_SLOTS slots of
    // [xy : LC_BATCH x nf x 2 floats | desc : LC_BATCH x nf x 8 words | n : LC_BATCH ints], the buffers' own layout -- three
    // copies per group and no wait for the stream (a wait per group kept host and device taking turns)
    uint8_t *gstage = nullptr;
    std::vector<hipEvent_t> gstage_ev;
    long gstage_next = 0;
    // what the last collected verdict was formed from (svo_lc_collect_ex)
    std::vector<int> last_cand_id;
    std::vector<double> last_cand_score;
    double last_ns = 0;
    // Verdicts formed AHEAD of their collection (round 5): when a frame is collected, the host logic runs for every
    // queued frame whose record has already landed (up to LC_AHEAD), and the geometric checks they need are one chain of
    // launches on the detector's own stream (lc_geom_launch) -- one wait per group instead of two per frame, and that wait
    // comes after the next group's chain has been started (Flight, below).  decided = n_host.size().
    struct Verdict {
        int entry = 0, status = 0, match = -1, nq = 0;
        bool need_geom = false, ransac = false;
        int old = -1, n_pairs = 0;
        std::vector<int> cand_id;
        std::vector<double> cand_score;
        double ns = 0;
    };
    std::deque<Verdict> verdicts;            // decided, not yet handed out
    DevBuf geo_dev;                          // per look-ahead slot: nearest / second-nearest arrays, the pairs, mask, result
    uint8_t *geo_host = nullptr;             // pinned, per slot: those arrays and the two key arrays on the host
    DevBuf geo_up;                           // the host block's first part on the device: the pairs of every check in one copy
    // The geometric checks run on a context (stream, RANSAC scratch) of the detector's own, behind the mark of the group of
    // frames they belong to: a collect waits for THAT group and for its checks, not for everything queued behind them -- the
    // feature extraction and scoring of the later frames keep the device busy meanwhile.
    svo_ctx *geo_ctx = nullptr;
    struct Mark {
        int end_entry;      // entries below it were complete on the detector's stream when the event fired
        hipEvent_t ev;
    };
    std::deque<Mark> marks;
    std::vector<hipEvent_t> free_events;
    // Groups whose verdicts are formed and whose geometric checks are on the device: up to two, so that a collect launches the
    // checks of the NEXT group before it waits for the oldest one's (which have had a group's worth of collects to finish).
    struct Flight {
        std::vector<Verdict> group;
        std::vector<int> slot_of;   // per verdict: its check's slot in the flight's half of the geo buffers, or -1
        int n_geo = 0, half = 0;
        hipEvent_t done = nullptr;  // recorded behind the chain of launches (n_geo > 0)
    };
    std::deque<Flight> flights;
    int next_half = 0;
    int in_flight() const
    {
        int n = 0;
        for (const Flight &f : flights)
            n += (int)f.group.size();
        return n;
    }
};
constexpr int LC_AHEAD = 16;
static_assert(LC_AHEAD <= SVO_LK_MAX_JOBS, "the geometric checks of a look-ahead group are one batched F-RANSAC launch");

extern "C" {

void svo_lc_default_params(svo_lc_params *p)
{
    if (!p)
        return;
    p->n_features = 500;          // cv::ORB::create() default
    p->fast_threshold = 20;
    p->hamming_threshold = 64;
    p->max_entries = 8192;
    p->use_nss = 1;               // include/visualSLAM.h:122
    p->alpha = 0.9f;              // :123
    p->k = 1;                     // :124
    p->dislocal = 20;             // Parameters::set(1), include/TemplatedLoopDetector.h:552-568
    p->max_db_results = 50;
    p->min_nss_factor = 0.005f;
    p->min_matches_per_group = 1;
    p->max_intragroup_gap = 3;
    p->max_distance_between_groups = 3;
    p->max_distance_between_queries = 2;
    p->min_Fpoints = 12;
    p->max_ransac_iterations = 500;
    p->ransac_probability = 0.99;
    p->max_reprojection_error = 2.0;
    p->max_neighbor_ratio = 0.6;
    p->seed = 0;
    p->orb_shape = SVO_ORB_SHAPE_CV;   // ORB::create()'s own pyramid and pipeline (src/optimizationStuff.cpp:50-55)
    p->orb_levels = 8;
    p->orb_scale_factor = 1.2f;
}

int svo_lc_create(svo_ctx *ctx, const svo_lc_params *params, int width, int height, int channels, svo_lc **out)
{
    SVO_CHECK_ARG(ctx && out);
    *out = nullptr;
    svo_lc *l = new svo_lc();
    l->ctx = ctx;
    if (params)
        l->prm = *params;
    else
        svo_lc_default_params(&l->prm);
    const svo_lc_params &p = l->prm;
    // k < 0 would pass every frame that reaches the temporal check, an alpha outside [0, 1] (or a NaN, which fails both
    // comparisons) cuts the candidates at no fraction of the normalisation score: refused, as a negative dislocal is
    if (p.n_features < 8 || p.n_features > 2048 || p.max_entries < 2 || p.dislocal < 0 || p.max_db_results < 1 ||
        p.max_db_results > LC_MAX_CAND || p.k < 0 || !(p.alpha >= 0.f && p.alpha <= 1.f)) {
        delete l;
        svo_set_error("svo_lc_create: n_features in 8..2048, max_entries >= 2, dislocal >= 0, k >= 0, alpha in 0..1, max_db_results "
                      "in 1..%d (the candidate list of a query is cut there BEFORE removeLowScores and the islands)", LC_MAX_CAND);
        return SVO_ERR_ARG;
    }
    l->w = width;
    l->h = height;
    l->c = channels;
    l->nf = p.n_features;
    l->capacity = p.max_entries;
    const size_t nf = (size_t)l->nf, cap = (size_t)l->capacity;
    int rc = p.orb_shape == SVO_ORB_SHAPE_CV
                 ? svo_orb_cv_create(ctx, width, height, channels, p.n_features, p.fast_threshold, p.orb_levels, p.orb_scale_factor,
                                     LC_BATCH, ctx->has_pattern ? ctx->orb_pattern : nullptr, &l->orb_cv)
                 : svo_orb_create(ctx, width, height, channels, p.n_features, p.fast_threshold, &l->orb);
    if (rc || (rc = l->db_desc.ensure(cap * nf * 32)) || (rc = l->db_xy.ensure(cap * nf * 8)) ||
        (rc = l->db_n.ensure(cap * 4)) || (rc = l->q.ensure((size_t)LC_BATCH * nf * (8 + 4 + 4 + 8 + 32) + LC_BATCH * 4 + 64)) ||
        (rc = l->counts.ensure(cap * 4)) || (rc = l->nn.ensure(nf * 12)) ||
        (rc = l->img.ensure((size_t)width * height * channels))) {
        svo_lc_destroy(l);
        return rc;
    }
    if (hipHostMalloc(reinterpret_cast<void **>(&l->rec), sizeof(LcRecord) * cap, hipHostMallocDefault) != hipSuccess) {
        svo_set_error("svo_lc_create: cannot pin %zu bytes for the per-frame records", sizeof(LcRecord) * cap);
        svo_lc_destroy(l);
        return SVO_ERR_HIP;
    }
    memset(l->rec, 0, sizeof(LcRecord) * cap);
    *out = l;
    return SVO_OK;
}

int svo_lc_destroy(svo_lc *l)
{
    if (!l)
        return SVO_OK;
    (void)hipStreamSynchronize(l->ctx->stream);
    if (l->geo_ctx) {
        (void)hipStreamSynchronize(l->geo_ctx->stream);
        svo_ctx_destroy(l->geo_ctx);
    }
    for (auto &m : l->marks)
        (void)hipEventDestroy(m.ev);
    for (auto &f : l->flights)
        if (f.done)
            (void)hipEventDestroy(f.done);
    for (hipEvent_t e : l->free_events)
        (void)hipEventDestroy(e);
    if (l->orb)
        svo_orb_destroy(l->orb);
    if (l->orb_cv)
        svo_orb_cv_destroy(l->orb_cv);
    if (l->rec)
        (void)hipHostFree(l->rec);
    if (l->rec_bow)
        (void)hipHostFree(l->rec_bow);
    if (l->stage)
        (void)hipHostFree(l->stage);
    if (l->gstage)
        (void)hipHostFree(l->gstage);
    for (hipEvent_t e : l->gstage_ev)
        if (e)
            (void)hipEventDestroy(e);
    if (l->geo_host)
        (void)hipHostFree(l->geo_host);
    l->geo_dev.release();
    l->geo_up.release();
    for (hipEvent_t e : l->stage_ev)
        if (e)
            (void)hipEventDestroy(e);
    DevBuf *bufs[] = {&l->db_desc, &l->db_xy, &l->db_n, &l->q, &l->counts, &l->nn, &l->img, &l->bw_w, &l->bw_v, &l->bw_nw, &l->bw_node,
                      &l->bw_head, &l->bw_next, &l->bw_plane, &l->bw_sums, &l->bw_mask, &l->q_word, &l->q_weight, &l->q_node};
    for (DevBuf *b : bufs)
        b->release();
    delete l;
    return SVO_OK;
}

int svo_lc_size(const svo_lc *l) { return l ? l->submitted : 0; }

// the query buffers of a frame: key points, octaves, responses, orientation vectors, descriptors, the live count
struct LcQuery {
    float *xy;
    int *oct;
    float *resp, *dir;
    uint32_t *desc;
    int *d_n;
};
// the buffers hold LC_BATCH frames, every array frame after frame (xy[g][nf][2], ..., n[g]): a batch's features are
// contiguous per array, so they enter the database in one copy per array
static LcQuery lc_query(svo_lc *l, int g = 0)
{
    const size_t nf = (size_t)l->nf, G = LC_BATCH;
    LcQuery q;
    float *xy0 = l->q.as<float>();
    int *oct0 = reinterpret_cast<int *>(xy0 + 2 * nf * G);
    float *resp0 = reinterpret_cast<float *>(oct0 + nf * G), *dir0 = resp0 + nf * G;
    uint32_t *desc0 = reinterpret_cast<uint32_t *>(dir0 + 2 * nf * G);
    int *n0 = reinterpret_cast<int *>(desc0 + 8 * nf * G);
    q.xy = xy0 + 2 * nf * g;
    q.oct = oct0 + nf * g;
    q.resp = resp0 + nf * g;
    q.dir = dir0 + 2 * nf * g;
    q.desc = desc0 + 8 * nf * g;
    q.d_n = n0 + g;
    return q;
}

// The features of G consecutive frames are in the query buffers (on the detector's stream): scoring against the database,
// the frames' own entries, the reduction of the scores to what the host logic reads.  Nothing is waited for.
// Vocabulary mode, every stage ONE launch for the G frames: a frame's candidates end `dislocal` entries before it and G <=
// dislocal, so no frame of the group can be another's candidate; the only thing frame f needs of the group is the score
// against entry f - 1 (the normalisation, :733) -- the rows of the whole group are linked into the inverted file FIRST, and
// every query reads its own column of sums (entries from the frame itself on are computed and never read).  Every double
// equals the frame-by-frame run's: a (word, entry) term does not depend on what else the lists hold.
static int lc_enqueue(svo_lc *l, int G = 1, bool query = true)
{
    svo_ctx *ctx = l->ctx;
    const svo_lc_params &p = l->prm;
    hipStream_t st = ctx->stream;
    const int entry0 = l->submitted;
    const size_t nf = (size_t)l->nf;
    const LcQuery q = lc_query(l);
    const int k_want = p.max_db_results < LC_MAX_CAND ? p.max_db_results : LC_MAX_CAND;
    int rc;
    if (l->voc) {
        // ---- DBoW2's way: BowVector + direct index of the frames (their database rows), queries through the inverted file ----
        int *row_w = l->bw_w.as<int>() + (size_t)entry0 * nf, *row_n = l->bw_nw.as<int>() + entry0;
        double *row_v = l->bw_v.as<double>() + (size_t)entry0 * nf;
        int *row_node = l->bw_node.as<int>() + (size_t)entry0 * nf;
        for (int g = 0; g < G; g++)
            l->rec_bow[entry0 + g].ready = 0;
        if ((rc = svo_voc_launch_transform(l->voc, st, q.desc, l->nf, q.d_n, l->di_levels, l->q_word.as<int>(),
                                           l->q_weight.as<double>(), l->q_node.as<int>(), G)) ||
            (rc = svo_bow_launch_vector(st, l->q_word.as<int>(), l->q_weight.as<double>(), l->q_node.as<int>(), l->nf, q.d_n, row_w,
                                        row_v, row_n, row_node, G)) ||
            (rc = svo_bow_launch_link(st, row_w, row_n, l->nf, entry0 * l->nf, l->bw_head.as<int>(), l->bw_next.as<int>(), G)) ||
            (query && (rc = svo_bow_launch_query(st, row_w, row_v, row_n, l->nf, l->bw_head.as<int>(), l->bw_next.as<int>(),
                                                 l->bw_v.as<double>(), l->nf, entry0 + G, l->bw_plane.as<double>(), l->capacity,
                                                 l->bw_sums.as<double>(), p.dislocal, k_want, entry0, q.d_n, l->rec_bow + entry0, G, l->bw_mask.as<unsigned>()))))
            return rc;
    }
    for (int g = 0; g < G && !l->voc; g++) {
        const int entry_id = entry0 + g;
        const LcQuery qg = lc_query(l, g);
        const int max_id = entry_id > p.dislocal ? entry_id - p.dislocal : 0;
        if (entry_id > 0 && query) {
            // ---- similarity of the query to every stored entry (one workgroup per entry) ----
            hipLaunchKernelGGL(lc_score_kernel, dim3(entry_id), dim3(256), nf * 32, st, qg.desc, qg.d_n, l->db_desc.as<uint32_t>(),
                               l->db_n.as<int>(), l->nf, p.hamming_threshold, l->counts.as<int>());
        }
        // ---- the query becomes entry `entry_id` (m_database->add + m_image_keys/descriptors, :728,:842-851) ----
        SVO_HIP(hipMemcpyAsync(l->db_desc.as<uint32_t>() + (size_t)entry_id * nf * 8, qg.desc, nf * 32, hipMemcpyDeviceToDevice, st));
        SVO_HIP(hipMemcpyAsync(l->db_xy.as<float>() + (size_t)entry_id * nf * 2, qg.xy, nf * 8, hipMemcpyDeviceToDevice, st));
        SVO_HIP(hipMemcpyAsync(l->db_n.as<int>() + entry_id, qg.d_n, 4, hipMemcpyDeviceToDevice, st));
        // ---- the <= max_db_results best entries below `dislocal`, the normalisation count, the feature count ----
        l->rec[entry_id].ready = 0;
        if (query)
            hipLaunchKernelGGL(lc_topk_kernel, dim3(1), dim3(256), 0, st, l->counts.as<int>(), max_id, k_want, qg.d_n, entry_id, l->nf,
                           l->rec + entry_id);
    }
    if (l->voc) {
        // ---- the queries become entries entry0 ... (m_database->add + m_image_keys/descriptors, :728,:842-851): one copy per array
        SVO_HIP(hipMemcpyAsync(l->db_desc.as<uint32_t>() + (size_t)entry0 * nf * 8, q.desc, (size_t)G * nf * 32, hipMemcpyDeviceToDevice, st));
        SVO_HIP(hipMemcpyAsync(l->db_xy.as<float>() + (size_t)entry0 * nf * 2, q.xy, (size_t)G * nf * 8, hipMemcpyDeviceToDevice, st));
        SVO_HIP(hipMemcpyAsync(l->db_n.as<int>() + entry0, q.d_n, (size_t)G * 4, hipMemcpyDeviceToDevice, st));
    }
    SVO_HIP(hipGetLastError());
    l->submitted = entry0 + G;
    // the mark of this group: its records, database rows and direct index are complete when it fires
    hipEvent_t ev;
    if (!l->free_events.empty()) {
        ev = l->free_events.back();
        l->free_events.pop_back();
    } else {
        SVO_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    }
    if (hipEventRecord(ev, st) != hipSuccess) {
        l->free_events.push_back(ev);
        svo_set_error("svo_lc: hipEventRecord failed");
        return SVO_ERR_HIP;
    }
    l->marks.push_back({l->submitted, ev});
    return SVO_OK;
}

static int lc_check_room(svo_lc *l, int n = 1)
{
    if (l->submitted + n > l->capacity) {
        svo_set_error("loop detector database is full (%d entries)", l->capacity);
        return SVO_ERR_STATE;
    }
    return SVO_OK;
}

// Queue one frame: features, scoring against the database, the frame's own entry, the reduction of the scores to what the
// host logic reads.  Nothing is waited for: the work runs on the detector's context -- give the detector a context of its
// own and it runs beside the front-end's streams.  With SVO_MEM_DEVICE the image is read by that queued work: it must
// stay valid until svo_lc_collect of this frame has returned.
int svo_lc_submit(svo_lc *l, const uint8_t *image, int mem)
{
    SVO_CHECK_ARG(l && image);
    SVO_CHECK_ARG(mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE);
    svo_ctx *ctx = l->ctx;
    SVO_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    int rc = lc_check_room(l);
    if (rc)
        return rc;
    const uint8_t *d_img = image;
    if (mem == SVO_MEM_HOST) {
        SVO_HIP(hipMemcpyAsync(l->img.p, image, (size_t)l->w * l->h * l->c, hipMemcpyHostToDevice, st));
        d_img = l->img.as<uint8_t>();
    }
    const LcQuery q = lc_query(l);
    if (l->orb_cv)
        rc = svo_orb_cv_launch(l->orb_cv, &d_img, 1, l->nf, q.xy, q.oct, q.resp, q.dir, q.desc, q.d_n, st);
    else
        rc = svo_orb_launch(l->orb, d_img, q.xy, q.oct, q.resp, q.dir, q.desc, q.d_n);
    if (rc)
        return rc;
    return lc_enqueue(l);
}

// n frames at once: the features of up to 16 images come out of ONE set of launches (orb_cv.hip) and, with a vocabulary, so
// does every stage of their scoring (lc_enqueue).  The verdicts are those of n svo_lc_submit calls, collected one by one as
// ever.  Device images must stay valid until the last of the frames has been collected; host images are staged.
int svo_lc_submit_batch(svo_lc *l, const uint8_t *const *images, int n, int mem)
{
    SVO_CHECK_ARG(l && images && n >= 0);
    SVO_CHECK_ARG(mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE);
    svo_ctx *ctx = l->ctx;
    SVO_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    int rc = lc_check_room(l, n);
    if (rc)
        return rc;
    const int group = l->orb_cv && l->voc ? (LC_BATCH < l->prm.dislocal ? LC_BATCH : (l->prm.dislocal > 1 ? l->prm.dislocal : 1)) : 1;
    if (group == 1) {
        for (int i = 0; i < n; i++)
            if ((rc = svo_lc_submit(l, images[i], mem)))
                return rc;
        return SVO_OK;
    }
    const size_t img_bytes = (size_t)l->w * l->h * l->c;
    if (mem == SVO_MEM_HOST && (rc = l->img.ensure(img_bytes * group)))
        return rc;
    for (int first = 0; first < n; first += group) {
        const int G = n - first < group ? n - first : group;
        const uint8_t *ptrs[LC_BATCH];
        for (int g = 0; g < G; g++) {
            ptrs[g] = images[first + g];
            if (mem == SVO_MEM_HOST) {
                uint8_t *slot = l->img.as<uint8_t>() + img_bytes * g;
                SVO_HIP(hipMemcpyAsync(slot, images[first + g], img_bytes, hipMemcpyHostToDevice, st));
                ptrs[g] = slot;
            }
        }
        const LcQuery q = lc_query(l);
        if ((rc = svo_orb_cv_launch(l->orb_cv, ptrs, G, l->nf, q.xy, q.oct, q.resp, q.dir, q.desc, q.d_n, st)) || (rc = lc_enqueue(l, G)))
            return rc;
    }
    return SVO_OK;
}

// the same for a frame whose features were extracted elsewhere (svo_orb_extract on another rank of a chunk-sharded run)
int svo_lc_submit_features(svo_lc *l, const float *xy, const uint32_t *desc, int n, int mem)
{
    SVO_CHECK_ARG(l && n >= 0 && n <= l->nf && (n == 0 || (xy && desc)));
    SVO_CHECK_ARG(mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE);
    svo_ctx *ctx = l->ctx;
    SVO_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    int rc = lc_check_room(l);
    if (rc)
        return rc;
    const LcQuery q = lc_query(l);
    SVO_HIP(hipMemsetAsync(q.xy, 0, (size_t)l->nf * 8, st));
    SVO_HIP(hipMemsetAsync(q.desc, 0, (size_t)l->nf * 32, st));
    if (n > 0 && mem == SVO_MEM_DEVICE) {
        SVO_HIP(hipMemcpyAsync(q.xy, xy, (size_t)n * 8, hipMemcpyDeviceToDevice, st));
        SVO_HIP(hipMemcpyAsync(q.desc, desc, (size_t)n * 32, hipMemcpyDeviceToDevice, st));
    } else if (n > 0) {
        // host arrays go through a ring of pinned slots, so that the call returns without waiting for the stream: a slot is
        // reused only when the copy that read it has run (its event)
        constexpr int SLOTS = 32;
        const size_t slot_bytes = (size_t)l->nf * 40;
        if (!l->stage) {
            // all or nothing: a ring whose events could not all be made is taken down again, not used half-built
            uint8_t *ring = nullptr;
            SVO_HIP(hipHostMalloc(reinterpret_cast<void **>(&ring), slot_bytes * SLOTS, hipHostMallocDefault));
            std::vector<hipEvent_t> evs(SLOTS, nullptr);
            hipError_t ee = hipSuccess;
            for (hipEvent_t &e : evs)
                if ((ee = hipEventCreateWithFlags(&e, hipEventDisableTiming)) != hipSuccess)
                    break;
            if (ee != hipSuccess) {
                for (hipEvent_t e : evs)
                    if (e)
                        (void)hipEventDestroy(e);
                (void)hipHostFree(ring);
                svo_set_error("svo_lc_submit_features: hipEventCreateWithFlags -> %s", hipGetErrorString(ee));
                return SVO_ERR_HIP;
            }
            l->stage = ring;
            l->stage_ev.swap(evs);
        }
        const int slot = l->stage_next++ % SLOTS;
        if (l->stage_next > SLOTS)
            SVO_HIP(hipEventSynchronize(l->stage_ev[slot]));
        uint8_t *h = l->stage + slot_bytes * slot;
        memcpy(h, xy, (size_t)n * 8);
        memcpy(h + (size_t)l->nf * 8, desc, (size_t)n * 32);
        SVO_HIP(hipMemcpyAsync(q.xy, h, (size_t)n * 8, hipMemcpyHostToDevice, st));
        SVO_HIP(hipMemcpyAsync(q.desc, h + (size_t)l->nf * 8, (size_t)n * 32, hipMemcpyHostToDevice, st));
        SVO_HIP(hipEventRecord(l->stage_ev[slot], st));
    }
    hipLaunchKernelGGL(lc_store_int_kernel, dim3(1), dim3(1), 0, st, q.d_n, n);  // the count travels as a kernel argument
    return lc_enqueue(l);
}

// n_frames frames given by their features, `cap` slots per frame in xy / desc (cap >= every n[g]); groups of up to 16 frames
// go through the scoring in one set of launches (vocabulary mode; else frame by frame)
static int lc_features_batch(svo_lc *l, const float *xy, const uint32_t *desc, const int *n, int n_frames, int cap, int mem, bool query)
{
    SVO_CHECK_ARG(l && n_frames >= 0 && cap >= 0 && (n_frames == 0 || (xy && desc && n)));
    SVO_CHECK_ARG(mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE);
    svo_ctx *ctx = l->ctx;
    SVO_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    int rc = lc_check_room(l, n_frames);
    if (rc)
        return rc;
    std::vector<int> hn(n_frames);
    if (mem == SVO_MEM_DEVICE) {
        SVO_HIP(hipMemcpyAsync(hn.data(), n, (size_t)n_frames * 4, hipMemcpyDeviceToHost, st));
        SVO_HIP(hipStreamSynchronize(st));
    } else {
        memcpy(hn.data(), n, (size_t)n_frames * 4);
    }
    for (int g = 0; g < n_frames; g++)
        SVO_CHECK_ARG(hn[g] >= 0 && hn[g] <= l->nf && hn[g] <= cap);
    const int group = l->voc ? (LC_BATCH < l->prm.dislocal ? LC_BATCH : (l->prm.dislocal > 1 ? l->prm.dislocal : 1)) : 1;
    const size_t nf = (size_t)l->nf;
    constexpr int GROUP_SLOTS = 3;
    const size_t gslot_bytes = (size_t)LC_BATCH * nf * 40 + 256;
    if (mem == SVO_MEM_HOST && !l->gstage) {
        // all or nothing, as the single-frame ring
        uint8_t *ring = nullptr;
        SVO_HIP(hipHostMalloc(reinterpret_cast<void **>(&ring), gslot_bytes * GROUP_SLOTS, hipHostMallocDefault));
        std::vector<hipEvent_t> evs(GROUP_SLOTS, nullptr);
        hipError_t ee = hipSuccess;
        for (hipEvent_t &e : evs)
            if ((ee = hipEventCreateWithFlags(&e, hipEventDisableTiming)) != hipSuccess)
                break;
        if (ee != hipSuccess) {
            for (hipEvent_t e : evs)
                if (e)
                    (void)hipEventDestroy(e);
            (void)hipHostFree(ring);
            svo_set_error("svo_lc_submit_features_batch: hipEventCreateWithFlags -> %s", hipGetErrorString(ee));
            return SVO_ERR_HIP;
        }
        l->gstage = ring;
        l->gstage_ev.swap(evs);
    }
    for (int first = 0; first < n_frames; first += group) {
        const int G = n_frames - first < group ? n_frames - first : group;
        const LcQuery q = lc_query(l);
        if (mem == SVO_MEM_HOST) {
            // through a pinned slot in the buffers' layout (unused entries zero): the call does not wait for the stream
            const int slot = (int)(l->gstage_next++ % GROUP_SLOTS);
            if (l->gstage_next > GROUP_SLOTS)
                SVO_HIP(hipEventSynchronize(l->gstage_ev[slot]));
            uint8_t *h = l->gstage + gslot_bytes * slot;
            float *hxy = reinterpret_cast<float *>(h);
            uint32_t *hdesc = reinterpret_cast<uint32_t *>(h + (size_t)LC_BATCH * nf * 8);
            int *hcount = reinterpret_cast<int *>(h + (size_t)LC_BATCH * nf * 40);
            for (int g = 0; g < G; g++) {
                const size_t f = (size_t)(first + g), k = (size_t)hn[f];
                memcpy(hxy + 2 * nf * g, xy + f * cap * 2, k * 8);
                memset(hxy + 2 * nf * g + 2 * k, 0, (nf - k) * 8);
                memcpy(hdesc + 8 * nf * g, desc + f * cap * 8, k * 32);
                memset(hdesc + 8 * nf * g + 8 * k, 0, (nf - k) * 32);
                hcount[g] = hn[f];
            }
            SVO_HIP(hipMemcpyAsync(q.xy, hxy, (size_t)G * nf * 8, hipMemcpyHostToDevice, st));
            SVO_HIP(hipMemcpyAsync(q.desc, hdesc, (size_t)G * nf * 32, hipMemcpyHostToDevice, st));
            SVO_HIP(hipMemcpyAsync(q.d_n, hcount, (size_t)G * 4, hipMemcpyHostToDevice, st));
            SVO_HIP(hipEventRecord(l->gstage_ev[slot], st));
        } else {
            SVO_HIP(hipMemsetAsync(q.xy, 0, (size_t)G * nf * 8, st));
            SVO_HIP(hipMemsetAsync(q.desc, 0, (size_t)G * nf * 32, st));
            if ((size_t)cap == nf) {   // the caller's layout is the buffers': one copy per array
                SVO_HIP(hipMemcpyAsync(q.xy, xy + (size_t)first * cap * 2, (size_t)G * nf * 8, hipMemcpyDeviceToDevice, st));
                SVO_HIP(hipMemcpyAsync(q.desc, desc + (size_t)first * cap * 8, (size_t)G * nf * 32, hipMemcpyDeviceToDevice, st));
            } else {
                for (int g = 0; g < G; g++) {
                    const size_t f = (size_t)(first + g);
                    if (hn[f] == 0)
                        continue;
                    SVO_HIP(hipMemcpyAsync(q.xy + 2 * nf * g, xy + f * cap * 2, (size_t)hn[f] * 8, hipMemcpyDeviceToDevice, st));
                    SVO_HIP(hipMemcpyAsync(q.desc + 8 * nf * g, desc + f * cap * 8, (size_t)hn[f] * 32, hipMemcpyDeviceToDevice, st));
                }
            }
            // the counts were read back above: they go down again from the call's own vector (a small pageable copy: the
            // runtime has taken the bytes when the call returns)
            SVO_HIP(hipMemcpyAsync(q.d_n, hn.data() + first, (size_t)G * 4, hipMemcpyHostToDevice, st));
        }
        if ((rc = lc_enqueue(l, G, query)))
            return rc;
        if (!query) {   // entries that were never queries: nothing to collect, they are part of the database at once
            for (int g = 0; g < G; g++)
                l->n_host.push_back(hn[first + g]);
            if (l->prm.use_nss && l->submitted > l->prm.dislocal)
                l->have_last = true;
        }
    }
    return SVO_OK;
}

int svo_lc_submit_features_batch(svo_lc *l, const float *xy, const uint32_t *desc, const int *n, int n_frames, int cap, int mem)
{
    return lc_features_batch(l, xy, desc, n, n_frames, cap, mem, true);
}

// Entries that enter the database WITHOUT being queries (no scoring, no verdict, nothing to collect): how a rank of a
// chunk-sharded run brings its detector to the state "every frame before my share has been seen" before it queues its own
// frames (chunked.py: sharded_detect).  Refused while queued frames wait to be collected (entries are collected in order).
int svo_lc_fill_features_batch(svo_lc *l, const float *xy, const uint32_t *desc, const int *n, int n_frames, int cap, int mem)
{
    SVO_CHECK_ARG(l);
    if (l->submitted != (int)l->n_host.size() || !l->verdicts.empty() || !l->flights.empty()) {
        svo_set_error("svo_lc_fill_features_batch: %d queued frame(s) have not been collected", svo_lc_pending(l));
        return SVO_ERR_STATE;
    }
    return lc_features_batch(l, xy, desc, n, n_frames, cap, mem, false);
}

int svo_lc_set_vocabulary(svo_lc *l, svo_voc *voc, int di_levels)
{
    SVO_CHECK_ARG(l && voc && di_levels >= 0);
    if (svo_voc_device_internal(voc) != l->ctx->device) {   // its arrays are read by this detector's kernels
        svo_set_error("svo_lc_set_vocabulary: the vocabulary lives on device %d, the detector on device %d",
                      svo_voc_device_internal(voc), l->ctx->device);
        return SVO_ERR_ARG;
    }
    if (l->submitted != 0) {
        svo_set_error("svo_lc_set_vocabulary: the database already holds %d entries", l->submitted);
        return SVO_ERR_STATE;
    }
    SVO_HIP(hipSetDevice(l->ctx->device));
    const size_t nf = (size_t)l->nf, cap = (size_t)l->capacity, nw = (size_t)svo_voc_words_internal(voc);
    if (cap > 16384) {
        svo_set_error("svo_lc_set_vocabulary: the candidate selection holds at most 16384 entries (max_entries %zu)", cap);
        return SVO_ERR_ARG;
    }
    int rc;
    if ((rc = l->bw_w.ensure(cap * nf * 4)) || (rc = l->bw_v.ensure(cap * nf * 8)) || (rc = l->bw_nw.ensure(cap * 4)) ||
        (rc = l->bw_node.ensure(cap * nf * 4)) || (rc = l->bw_head.ensure((nw + 1) * 4)) || (rc = l->bw_next.ensure(cap * nf * 4 * 6)) ||
        (rc = l->bw_plane.ensure((size_t)LC_BATCH * nf * cap * 8)) || (rc = l->bw_sums.ensure((size_t)LC_BATCH * cap * 8)) ||
        (rc = l->bw_mask.ensure((size_t)LC_BATCH * cap * svo_bow_mask_words(l->nf) * 4)) ||
        (rc = l->q_word.ensure((size_t)LC_BATCH * nf * 4)) || (rc = l->q_weight.ensure((size_t)LC_BATCH * nf * 8)) ||
        (rc = l->q_node.ensure((size_t)LC_BATCH * nf * 4)))
        return rc;
    SVO_HIP(hipMemset(l->bw_head.p, 0xff, (nw + 1) * 4));
    SVO_HIP(hipMemset(l->bw_next.p, 0xff, cap * nf * 4 * 6));  // six skip pointers per row slot (bow.hip: BOW_SKIPS)
    SVO_HIP(hipMemset(l->bw_sums.p, 0, (size_t)LC_BATCH * cap * 8));
    SVO_HIP(hipMemset(l->bw_mask.p, 0, (size_t)LC_BATCH * cap * svo_bow_mask_words(l->nf) * 4));
    if (!l->rec_bow) {
        if (hipHostMalloc(reinterpret_cast<void **>(&l->rec_bow), sizeof(svo_lc_bow_record) * cap, hipHostMallocDefault) != hipSuccess) {
            svo_set_error("svo_lc_set_vocabulary: cannot pin %zu bytes for the per-frame records", sizeof(svo_lc_bow_record) * cap);
            return SVO_ERR_HIP;
        }
        memset(l->rec_bow, 0, sizeof(svo_lc_bow_record) * cap);
    }
    l->voc = voc;
    l->di_levels = di_levels;
    return SVO_OK;
}

int svo_lc_pending(const svo_lc *l) { return l ? l->submitted - (int)l->n_host.size() + (int)l->verdicts.size() + l->in_flight() : 0; }

// The host logic of detectLoop for entry `entry_id`, whose record has landed: everything up to the geometric check, which is
// only REQUESTED here (v.need_geom, v.old) -- the temporal window does not depend on its outcome (:966-1003 run before it).
static int lc_decide(svo_lc *l, int entry_id, svo_lc::Verdict &v)
{
    const svo_lc_params &p = l->prm;
    const bool bow = l->voc != nullptr;
    // the candidates of the database query (score descending, entry id ascending on ties -- what the sort of the
    // id-ordered result list gives) and the normalisation score
    std::vector<Result> qret;
    double ns_have = 0.;
    int nq = 0;  // features of the query (0 features: no geometric check possible)
    if (bow) {
        // DBoW2: score = -(sum over the common words of |v - w| - |v| - |w|) / 2 (TemplatedDatabase::queryL1,
        // L1Scoring::score for the normalisation against the previous frame's vector, :733)
        const svo_lc_bow_record &rec = l->rec_bow[entry_id];
        for (int k = 0; k < rec.n_cand; k++)
            qret.push_back({rec.cand_id[k], -rec.cand_sum[k] / 2.0});
        ns_have = -rec.last_sum / 2.0;
        nq = rec.n_feat;
    } else {
        const LcRecord &rec = l->rec[entry_id];
        nq = rec.nq;
        auto score_of = [&](int count) { return nq > 0 ? (double)count / (double)nq : 0.; };
        for (int k = 0; k < rec.n_cand; k++)
            qret.push_back({rec.cand_id[k], score_of(rec.cand_count[k])});
        ns_have = score_of(rec.last_count);
    }
    std::sort(qret.begin(), qret.end(),
              [](const Result &a, const Result &b) { return a.score > b.score || (a.score == b.score && a.id < b.id); });
    if ((int)qret.size() > p.max_db_results)
        qret.resize(p.max_db_results);
    v.entry = entry_id;
    v.nq = nq;
    v.cand_id.clear();
    v.cand_score.clear();
    for (const Result &r : qret) {
        v.cand_id.push_back(r.id);
        v.cand_score.push_back(r.score);
    }
    v.ns = 0.;

    int st_out = SVO_LC_CLOSE_MATCHES_ONLY, match_out = -1;
    if (entry_id > p.dislocal) {  // :714-722
        if (!qret.empty()) {
            double ns = 1.0;
            if (p.use_nss)
                ns = l->have_last ? ns_have : 0.;  // :736-739
            v.ns = ns;
            if (!p.use_nss || ns >= p.min_nss_factor) {
                const double cut = (double)p.alpha * ns;  // removeLowScores, :1320-1338
                size_t keep = 0;
                while (keep < qret.size() && qret[keep].score >= cut)
                    keep++;
                qret.resize(keep);
                if (!qret.empty()) {
                    match_out = qret[0].id;
                    // ---- computeIslands, :875-951 ----
                    std::vector<Island> islands;
                    if (qret.size() == 1) {
                        islands.push_back({qret[0].id, qret[0].id, qret[0].score, qret[0].id, qret[0].score});
                    } else {
                        std::stable_sort(qret.begin(), qret.end(), [](const Result &a, const Result &b) { return a.id < b.id; });
                        int first = qret[0].id, last = qret[0].id;
                        size_t i_first = 0, i_last = 0;
                        double best_score = qret[0].score;
                        int best_entry = qret[0].id;
                        auto close = [&]() {
                            if (last - first + 1 >= p.min_matches_per_group) {
                                double sum = 0;
                                for (size_t i = i_first; i <= i_last; i++)
                                    sum += qret[i].score;
                                islands.push_back({first, last, sum, best_entry, best_score});
                            }
                        };
                        for (size_t idx = 1; idx < qret.size(); idx++) {
                            if (qret[idx].id - last < p.max_intragroup_gap) {
                                last = qret[idx].id;
                                i_last = idx;
                                if (qret[idx].score > best_score) {
                                    best_score = qret[idx].score;
                                    best_entry = qret[idx].id;
                                }
                            } else {
                                close();
                                first = last = qret[idx].id;
                                i_first = i_last = idx;
                                best_score = qret[idx].score;
                                best_entry = qret[idx].id;
                            }
                        }
                        close();
                    }
                    if (!islands.empty()) {
                        size_t bi = 0;  // std::max_element: the first maximum
                        for (size_t i = 1; i < islands.size(); i++)
                            if (islands[bi].score < islands[i].score)
                                bi = i;
                        const Island &isl = islands[bi];
                        // ---- updateTemporalWindow, :966-1003 ----
                        if (l->window_n == 0 || entry_id - l->window_query > p.max_distance_between_queries) {
                            l->window_n = 1;
                        } else {
                            const int a1 = l->window_first, a2 = l->window_last, b1 = isl.first, b2 = isl.last;
                            bool fit = (b1 <= a1 && a1 <= b2) || (a1 <= b1 && b1 <= a2);
                            if (!fit) {
                                const int d1 = a1 - b2, d2 = b1 - a2;
                                fit = (d1 > d2 ? d1 : d2) <= p.max_distance_between_groups;
                            }
                            l->window_n = fit ? l->window_n + 1 : 1;
                        }
                        l->window_first = isl.first;
                        l->window_last = isl.last;
                        l->window_query = entry_id;
                        match_out = isl.best_entry;
                        if (l->window_n > p.k) {
                            // ---- the geometric check is due: requested here, run by lc_geom_* (a frame without features on
                            // either side cannot pass it) ----
                            v.old = isl.best_entry;
                            v.need_geom = l->n_host[isl.best_entry] > 0 && nq > 0;
                            st_out = SVO_LC_NO_GEOMETRICAL_CONSISTENCY;   // until lc_geom_finish says otherwise
                        } else
                            st_out = SVO_LC_NO_TEMPORAL_CONSISTENCY;
                    } else
                        st_out = SVO_LC_NO_GROUPS;
                } else
                    st_out = SVO_LC_LOW_SCORES;
            } else
                st_out = SVO_LC_LOW_NSS_FACTOR;
        } else
            st_out = SVO_LC_NO_DB_RESULTS;
    }
    l->n_host.push_back(nq);
    if (p.use_nss && entry_id + 1 > p.dislocal)  // :855-858
        l->have_last = true;
    v.status = st_out;
    v.match = match_out;
    return SVO_OK;
}

// ---- the geometric check in three parts, so that the checks of several frames share their waits ----
// per look-ahead slot: device  [bj | d1 | d2 : 3 nf ints][p_old | p_cur : 2 x nf x 2 floats][mask : nf bytes, padded][F 9 doubles, count, iterations]
//                      host    [bj | d1 | d2][node of the old entry : nf ints][keys old | keys current : 2 x nf x 2 floats][F, count, iterations]
static size_t geo_dev_stride(const svo_lc *l) { return (((size_t)l->nf * (12 + 16 + 1) + 255) & ~(size_t)255) + 256; }
static size_t geo_host_stride(const svo_lc *l) { return (((size_t)l->nf * (12 + 4 + 16) + 255) & ~(size_t)255) + 256; }

static size_t geo_match_lds(const svo_lc *l) { return (size_t)l->nf * 28 + 64; }

static int lc_geom_ensure(svo_lc *l)
{
    if (geo_match_lds(l) > 64 * 1024) {
        svo_set_error("svo_lc: the geometric check holds a frame's matches in 64 KB of LDS: at most 2300 features per frame (%d)", l->nf);
        return SVO_ERR_ARG;
    }
    int rc = l->geo_dev.ensure(geo_dev_stride(l) * LC_AHEAD * 2);   // two halves: one per group in flight
    if (rc || (rc = l->geo_up.ensure(geo_host_stride(l) * LC_AHEAD * 2)) || (!l->geo_ctx && (rc = svo_ctx_create(l->ctx->device, &l->geo_ctx))))
        return rc;
    if (!l->geo_host)
        SVO_HIP(hipHostMalloc(reinterpret_cast<void **>(&l->geo_host), geo_host_stride(l) * LC_AHEAD * 2, hipHostMallocDefault));
    return SVO_OK;
}

// The geometric checks of a look-ahead group (slot k = the k-th of them), one chain of launches on the detector's own stream:
//   1. nearest / second-nearest current feature of every old feature (under a common direct-index node with a vocabulary,
//      isGeometricallyConsistent_DI :1005-1087; exhaustive without, :1101-1160);
//   2. the neighbour-ratio matches -> the pair lists, their counts and the RANSACs' gates (lc_geo_match_kernel);
//   3. the fundamental-matrix RANSACs of all the checks as ONE batched launch, each gated on min_Fpoints pairs
//      (DVision::FSolver::checkFundamentalMat is a RANSAC at any count: not findFundamentalMat's least-median branch below 15);
//   4. inlier counts and pair counts into the pinned block.
// The host waits once, for the whole chain.
static int lc_geom_launch(svo_lc *l, const std::vector<const svo_lc::Verdict *> &checks, int half)
{
    hipStream_t st = l->geo_ctx->stream;
    const svo_lc_params &p = l->prm;
    const size_t nf = (size_t)l->nf;
    const bool bow = l->voc != nullptr;
    const int n = (int)checks.size();
    LcGeoBatch gb;
    SvoDiBatch db;
    memset(&gb, 0, sizeof(gb));
    memset(&db, 0, sizeof(db));
    int na_max = 0, rc;
    for (int k = 0; k < n; k++) {
        gb.old_entry[k] = db.old_entry[k] = checks[k]->old;
        gb.cur_entry[k] = db.cur_entry[k] = checks[k]->entry;   // the query IS entry `entry` now
        gb.na[k] = db.na[k] = l->n_host[checks[k]->old];
        na_max = db.na[k] > na_max ? db.na[k] : na_max;
    }
    const size_t ds = geo_dev_stride(l), us = geo_host_stride(l);
    uint8_t *dev = l->geo_dev.as<uint8_t>() + ds * LC_AHEAD * half, *up = l->geo_up.as<uint8_t>() + us * LC_AHEAD * half;
    if (bow) {
        if ((rc = svo_bow_launch_di_nearest_batch(st, db, n, na_max, l->db_desc.as<uint32_t>(), l->bw_node.as<int>(), l->db_n.as<int>(),
                                                  l->nf, dev, ds)))
            return rc;
    } else {
        for (int k = 0; k < n; k++) {
            int *bj = reinterpret_cast<int *>(dev + ds * k), *dd1 = bj + nf, *dd2 = dd1 + nf;
            const int na = db.na[k];
            if (na > 0)
                hipLaunchKernelGGL(lc_nearest2_kernel, dim3((na + 255) / 256), dim3(256), nf * 32, st,
                                   l->db_desc.as<uint32_t>() + (size_t)db.old_entry[k] * nf * 8, na,
                                   l->db_desc.as<uint32_t>() + (size_t)db.cur_entry[k] * nf * 8, l->db_n.as<int>() + db.cur_entry[k], bj, dd1, dd2);
        }
    }
    hipLaunchKernelGGL(lc_geo_match_kernel, dim3(n), dim3(512), geo_match_lds(l), st, gb, l->nf, dev, ds,
                       bow ? l->bw_node.as<int>() : nullptr, l->db_xy.as<float>(), up, us, p.max_neighbor_ratio, p.min_Fpoints);
    SVO_HIP(hipGetLastError());
    svo_fransac_job jobs[LC_AHEAD];
    for (int k = 0; k < n; k++) {
        uint8_t *d = dev + ds * k;
        double *dF = reinterpret_cast<double *>(d + ds - 256);
        int *tail = reinterpret_cast<int *>(dF);
        svo_fransac_job &job = jobs[k];
        job = svo_fransac_job();
        job.p1 = reinterpret_cast<float *>(up + us * k);
        job.p2 = job.p1 + 2 * nf;
        job.cap = l->nf;
        job.d_n = tail + GEO_TAIL_PAIRS;
        job.gate = tail + GEO_TAIL_GATE;
        job.threshold = p.max_reprojection_error;
        job.confidence = p.ransac_probability;
        job.max_iters = p.max_ransac_iterations;
        job.seed = p.seed + (uint64_t)checks[k]->entry;
        job.mask = d + nf * 28;
        job.d_F = dF;
        job.d_count = tail + 18;
        job.d_iters = tail + 19;
        job.cv_small = false;
    }
    if ((rc = svo_launch_fransac_batch(l->geo_ctx, n, jobs)))
        return rc;
    hipLaunchKernelGGL(lc_geo_result_kernel, dim3(1), dim3(256), 0, st, n, dev, ds, l->geo_host + us * LC_AHEAD * half, us);
    SVO_HIP(hipGetLastError());
    return SVO_OK;
}

// after the wait: the verdict
static void lc_geom_finish(svo_lc *l, svo_lc::Verdict &v, int slot)   // slot: counted over both halves
{
    const uint8_t *h = l->geo_host + geo_host_stride(l) * slot;
    const int *tail = reinterpret_cast<const int *>(h + geo_host_stride(l) - 256);
    v.n_pairs = tail[GEO_TAIL_PAIRS];
    v.ransac = v.n_pairs >= l->prm.min_Fpoints;
    const bool detection = v.ransac && tail[18] >= l->prm.min_Fpoints;
    v.status = detection ? SVO_LC_LOOP_DETECTED : SVO_LC_NO_GEOMETRICAL_CONSISTENCY;
}

// The oldest queued frame's verdict: waits (on the DETECTOR's stream only) until its record has landed, then the host logic of
// detectLoop -- for this frame and for every later queued frame whose record has landed too (up to LC_AHEAD): their geometric
// checks are one chain of launches and one wait, and the following group's chain is started before that wait.  Frames are
// handed out in the order they were submitted.
int svo_lc_collect_ex(svo_lc *l, int *status, int *query, int *match, int *cand_id, double *cand_score, int cap_out,
                      int *n_cand_out, double *ns_factor)
{
    SVO_CHECK_ARG(l && status);
    svo_ctx *ctx = l->ctx;
    if (l->verdicts.empty()) {
        if ((int)l->n_host.size() >= l->submitted && l->flights.empty()) {
            svo_set_error("svo_lc_collect: no frame is queued");
            return SVO_ERR_STATE;
        }
        SVO_HIP(hipSetDevice(ctx->device));
        hipStream_t st = ctx->stream;
        const bool bow = l->voc != nullptr;
        auto landed = [&](int e) {
            const int *ready = bow ? &l->rec_bow[e].ready : &l->rec[e].ready;
            return __atomic_load_n(ready, __ATOMIC_ACQUIRE) == e + 1;
        };
        // marks of groups whose verdicts are all formed go back to the pool
        auto retire = [&]() {
            while (!l->marks.empty() && l->marks.front().end_entry <= (int)l->n_host.size()) {
                l->free_events.push_back(l->marks.front().ev);
                l->marks.pop_front();
            }
        };
        // form the verdicts of the landed frames from `first` on (up to LC_AHEAD) and start their geometric checks
        auto form = [&](int first) -> int {
            int rc;
            l->flights.emplace_back();
            svo_lc::Flight &f = l->flights.back();
            f.half = l->next_half;
            l->next_half ^= 1;
            for (int e = first; e < l->submitted && (int)f.group.size() < LC_AHEAD && landed(e); e++) {
                f.group.emplace_back();
                if ((rc = lc_decide(l, e, f.group.back())))
                    return rc;
                f.slot_of.push_back(f.group.back().need_geom ? f.n_geo++ : -1);
            }
            if (f.n_geo == 0)
                return SVO_OK;
            std::vector<const svo_lc::Verdict *> checks;
            for (size_t k = 0; k < f.group.size(); k++)
                if (f.slot_of[k] >= 0)
                    checks.push_back(&f.group[k]);
            if ((rc = lc_geom_ensure(l)))
                return rc;
            hipStream_t gst = l->geo_ctx->stream;
            // the checks read database rows up to the group's last entry: behind the mark that covers it (a record can land
            // before the copies that follow it in its group's launches)
            const int last_entry = f.group.back().entry;
            for (const auto &m : l->marks)
                if (m.end_entry > last_entry) {
                    SVO_HIP(hipStreamWaitEvent(gst, m.ev, 0));
                    break;
                }
            if ((rc = lc_geom_launch(l, checks, f.half)))
                return rc;
            if (!l->free_events.empty()) {
                f.done = l->free_events.back();
                l->free_events.pop_back();
            } else {
                SVO_HIP(hipEventCreateWithFlags(&f.done, hipEventDisableTiming));
            }
            SVO_HIP(hipEventRecord(f.done, gst));
            return SVO_OK;
        };
        int rc;
        retire();
        if (l->flights.empty()) {   // nothing under way: wait for the group the oldest queued frame belongs to
            const int first = (int)l->n_host.size();
            if (!landed(first)) {
                hipEvent_t ev = nullptr;
                for (const auto &m : l->marks)
                    if (m.end_entry > first) {
                        ev = m.ev;
                        break;
                    }
                if (ev)
                    SVO_HIP(hipEventSynchronize(ev));
                else
                    SVO_HIP(hipStreamSynchronize(st));
                if (!landed(first)) {
                    svo_set_error("svo_lc_collect: the record of entry %d did not arrive", first);
                    return SVO_ERR_HIP;
                }
            }
            if ((rc = form(first)))
                return rc;
        }
        // the next group's checks go out before the wait for this one's
        if (l->flights.size() < 2 && (int)l->n_host.size() < l->submitted && landed((int)l->n_host.size()) && (rc = form((int)l->n_host.size())))
            return rc;
        retire();
        svo_lc::Flight f = std::move(l->flights.front());
        l->flights.pop_front();
        if (f.n_geo > 0 && !f.done) {   // its chain of launches failed when it was formed (that call returned the error)
            svo_set_error("svo_lc_collect: the geometric checks of entries %d ... were not launched", f.group.empty() ? -1 : f.group.front().entry);
            return SVO_ERR_STATE;
        }
        if (f.n_geo > 0) {
            const hipError_t e = hipEventSynchronize(f.done);
            l->free_events.push_back(f.done);
            if (e != hipSuccess) {
                svo_set_error("svo_lc_collect: hipEventSynchronize -> %s", hipGetErrorString(e));
                return SVO_ERR_HIP;
            }
            for (size_t k = 0; k < f.group.size(); k++)
                if (f.slot_of[k] >= 0)
                    lc_geom_finish(l, f.group[k], LC_AHEAD * f.half + f.slot_of[k]);
        }
        for (auto &g : f.group)
            l->verdicts.push_back(std::move(g));
    }
    svo_lc::Verdict v = std::move(l->verdicts.front());
    l->verdicts.pop_front();
    l->last_cand_id = v.cand_id;
    l->last_cand_score = v.cand_score;
    l->last_ns = v.ns;
    *status = v.status;
    if (query)
        *query = v.entry;
    if (match)
        *match = v.match;
    if (n_cand_out)
        *n_cand_out = (int)l->last_cand_id.size();
    for (int k = 0; k < (int)l->last_cand_id.size() && k < cap_out; k++) {
        if (cand_id)
            cand_id[k] = l->last_cand_id[k];
        if (cand_score)
            cand_score[k] = l->last_cand_score[k];
    }
    if (ns_factor)
        *ns_factor = l->last_ns;
    return SVO_OK;
}

int svo_lc_collect(svo_lc *l, int *status, int *query, int *match)
{
    return svo_lc_collect_ex(l, status, query, match, nullptr, nullptr, 0, nullptr, nullptr);
}

int svo_lc_collect_batch(svo_lc *l, int n, int *status, int *query, int *match)
{
    SVO_CHECK_ARG(l && n >= 0 && (n == 0 || status));
    if (n > svo_lc_pending(l)) {
        svo_set_error("svo_lc_collect_batch: %d verdicts asked for, %d frame(s) queued", n, svo_lc_pending(l));
        return SVO_ERR_STATE;
    }
    for (int i = 0; i < n; i++) {
        const int rc = svo_lc_collect_ex(l, status + i, query ? query + i : nullptr, match ? match + i : nullptr, nullptr, nullptr, 0,
                                         nullptr, nullptr);
        if (rc)
            return rc;
    }
    return SVO_OK;
}

// submit + collect: the synchronous form, one call per frame, in order (checkLoopDetectorStatus as the reference
// calls it, src/optimizationStuff.cpp:49-64)
int svo_lc_detect(svo_lc *l, const uint8_t *image, int mem, int *status, int *query, int *match)
{
    SVO_CHECK_ARG(l && image && status);
    if (svo_lc_pending(l) != 0) {
        svo_set_error("svo_lc_detect: %d queued frames are not collected yet", svo_lc_pending(l));
        return SVO_ERR_STATE;
    }
    int rc = svo_lc_submit(l, image, mem);
    if (rc)
        return rc;
    return svo_lc_collect(l, status, query, match);
}

}  // extern "C"
