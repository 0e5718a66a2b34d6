// replenish.hip -- the duplicate filter of a tracked point set and the duplicate-aware top-up of that set, for gfx950.
//
// Replaces removeDuplicate and the replenishing step of VisOdometry.trackSequence (src/ROSslam.py:156-169, 262-271) and
// removeDuplicates (include/monoUtils.h:195-213).  The definition is the one tests/replenish_numpy.py states.
//
// Launches:
//   dedup_kernel    one new point per lane, workgroups of 256; the reference points (or the ref_idx gather of them) pass through LDS
//                   in tiles of 1024 and every lane tests the whole tile.  Brute force: the answer per new point is a boolean that
//                   does not depend on the order of the search.
//   append_kernel   svo_replenish only: single-wave workgroups as in geometry.hip's compact_kernel.  Wave w owns the w-th segment
//                   of the new points, counts the survivors (keep && z > 0, the transform recomputed) of the whole prefix itself and
//                   writes its own survivors, moved, behind them: order-preserving, no atomic decides a position.
#include <cmath>

#include "replenish_plan.hip.h"
#include "svo_internal.h"
#include "wave_ops.hip.h"

namespace {

using namespace replenish_plan;

// what a lane tests reference points against: BOX keeps the four limits, DISC the point and the radius
struct Probe {
    double xl, xh, yl, yh;   // BOX: qx - r, qx + r, qy - r, qy + r in double
    float qx, qy;            // DISC
};

template <int MODE> __device__ __forceinline__ bool near(const float2 p, const Probe &q, double r, double r2_hi)
{
    if (MODE == SVO_DEDUP_BOX) {
        const double rx = p.x, ry = p.y;
        return rx > q.xl && rx < q.xh && ry > q.yl && ry < q.yh;
    }
    const float dx = p.x - q.qx, dy = p.y - q.qy;            // Point2f::operator-
    const double s = (double)dx * dx + (double)dy * dy;      // no contraction (the file is built with -ffp-contract=off)
    // The decision is sqrt(s) < r.  The square root is monotone and r2_hi lies above r * r, so s >= r2_hi cannot pass it: the first
    // comparison only spares the square root of the pairs that are far apart, it decides nothing.
    return s < r2_hi && sqrt(s) < r;
}

template <int MODE>
__global__ __launch_bounds__(BLOCK) void dedup_kernel(const float2 *__restrict__ ref, int n_ref, const int *__restrict__ idx, int n_src,
                                                      const float2 *__restrict__ fresh, int n_new, double r, double r2_hi,
                                                      uint8_t *__restrict__ keep, int *__restrict__ n_keep)
{
    __shared__ float2 tile[TILE];
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    const bool live = i < n_new;
    const float2 q = live ? fresh[i] : make_float2(0.f, 0.f);
    Probe pr;
    pr.xl = (double)q.x - r, pr.xh = (double)q.x + r, pr.yl = (double)q.y - r, pr.yh = (double)q.y + r;
    pr.qx = q.x, pr.qy = q.y;
    bool dup = !live;   // a lane past the end has nothing to find: it never holds its wave back
    // The trip count comes from n_src (n_ref or n_idx) ALONE, a kernel argument: every wave of the workgroup reaches both barriers of
    // every tile.  A wave whose lanes are all settled skips a tile's COMPARES, never the loop or a barrier in it.
    const int n_tiles = (n_src + TILE - 1) / TILE;
    for (int t = 0; t < n_tiles; t++) {
        const int base = t * TILE;
        __syncthreads();   // the previous tile's readers are done
        for (int k = threadIdx.x; k < TILE; k += BLOCK) {
            const int j = base + k;
            // a slot with no reference point holds NaNs: every comparison with it is false
            float2 p = make_float2(__builtin_nanf(""), __builtin_nanf(""));
            if (j < n_src) {
                const int s = idx ? idx[j] : j;
                if ((unsigned)s < (unsigned)n_ref)   // an entry outside [0, n_ref) is skipped, nothing is read through it
                    p = ref[s];
            }
            tile[k] = p;
        }
        __syncthreads();
        const int cnt = min(TILE, n_src - base);
        for (int k0 = 0; k0 < cnt; k0 += 64) {        // no barrier in here: leaving early is free
            if (__ballot(!dup) == 0ull)
                break;
            const int k1 = min(k0 + 64, cnt);
            for (int k = k0; k < k1; k++)
                dup = dup || near<MODE>(tile[k], pr, r, r2_hi);
        }
    }
    // the prototype returns "x != 0" of the points it zeroed: a new point at x == 0 goes whatever its neighbours
    const bool kept = live && !dup && !(MODE == SVO_DEDUP_BOX && q.x == 0.f);
    if (live)
        keep[i] = kept ? 1 : 0;
    if (n_keep) {   // a count only: no order depends on it
        const unsigned long long m = __ballot(kept);
        if ((threadIdx.x & 63) == 0 && m)
            atomicAdd(n_keep, __popcll(m));
    }
}

// 1: appended, 0: a duplicate, -1: behind the camera.  out: the moved point.
__device__ __forceinline__ int survivor(const Mat34 &Rt, const uint8_t *__restrict__ keep, const float *__restrict__ xyz, int i, float (&out)[3])
{
    if (keep[i] != 1)
        return 0;
    const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
#pragma unroll
    for (int r = 0; r < 3; r++)   // transform_kernel's expression (geometry.hip)
        out[r] = (float)(Rt.m[4 * r] * x + Rt.m[4 * r + 1] * y + Rt.m[4 * r + 2] * z + Rt.m[4 * r + 3]);
    return out[2] > 0.f ? 1 : -1;
}

// out_xy / out_xyz: row n_ref of the reference arrays.  counts (optional): n_out, n_dup, n_behind.
__global__ __launch_bounds__(64) void append_kernel(Mat34 Rt, const uint8_t *__restrict__ keep, const float2 *__restrict__ fresh,
                                                    const float *__restrict__ xyz, int n_new, int seg, int n_ref,
                                                    float2 *__restrict__ out_xy, float *__restrict__ out_xyz, int *n_out, int *n_dup,
                                                    int *n_behind)
{
    svo_chain_priority();
    const int lane = threadIdx.x;
    const int first = blockIdx.x * seg;   // this wave's segment: [first, last)
    if (first >= n_new && !(n_new <= 0 && blockIdx.x == 0))
        return;
    const int last = min(first + seg, n_new);
    float moved[3];
    // survivors and duplicates before the segment
    int part = 0, part_dup = 0;
    for (int i = lane; i < first; i += 64) {
        const int s = survivor(Rt, keep, xyz, i, moved);
        part += s == 1 ? 1 : 0;
        part_dup += s == 0 ? 1 : 0;
    }
    int pos0 = __builtin_amdgcn_readfirstlane(svo::wave_sum(part));
    int dup0 = __builtin_amdgcn_readfirstlane(svo::wave_sum(part_dup));
    for (int start = first; start < last; start += 64) {
        const int i = start + lane;
        const int s = i < last ? survivor(Rt, keep, xyz, i, moved) : -2;
        const unsigned long long bal = __ballot(s == 1);
        if (s == 1) {
            const int pos = pos0 + __popcll(bal & ((1ull << lane) - 1ull));
            out_xy[pos] = fresh[i];
#pragma unroll
            for (int r = 0; r < 3; r++)
                out_xyz[(size_t)pos * 3 + r] = moved[r];
        }
        pos0 += __popcll(bal);
        dup0 += __popcll(__ballot(s == 0));
    }
    if (last >= n_new && lane == 0) {   // the wave that owns the end of the array
        if (n_out)
            *n_out = n_ref + pos0;
        if (n_dup)
            *n_dup = dup0;
        if (n_behind)
            *n_behind = (n_new > 0 ? n_new : 0) - dup0 - pos0;
    }
}

// p is never null (check_replenish refuses it); geometry.hip's to_mat34 differs: there null means "no transform", all zeros
Mat34 to_mat34(const double *p)
{
    Mat34 m;
    memcpy(m.m, p, sizeof(m.m));
    return m;
}

// a bound above r * r that the rounding of the product cannot fall below (see near<SVO_DEDUP_DISC>)
double radius2_above(double r)
{
    const double r2 = r * r;
    return r2 + (r2 * 0x1p-40 + 0x1p-1000);
}

// device pointers; d_keep: n_new bytes; d_n_keep: a device int or null
int launch_dedup(svo_ctx *ctx, const float *ref_xy, int n_ref, const int *ref_idx, int n_idx, const float *new_xy, int n_new,
                 double radius, int mode, uint8_t *d_keep, int *d_n_keep)
{
    hipStream_t st = ctx->stream;
    if (d_n_keep)
        SVO_HIP(hipMemsetAsync(d_n_keep, 0, sizeof(int), st));
    if (n_new <= 0)
        return SVO_OK;
    const int n_src = sources(n_ref, ref_idx, n_idx);
    const auto kernel = mode == SVO_DEDUP_BOX ? dedup_kernel<SVO_DEDUP_BOX> : dedup_kernel<SVO_DEDUP_DISC>;
    hipLaunchKernelGGL(kernel, dim3(blocks(n_new)), dim3(BLOCK), 0, st, reinterpret_cast<const float2 *>(ref_xy), n_ref, ref_idx, n_src,
                       reinterpret_cast<const float2 *>(new_xy), n_new, radius, radius2_above(radius), d_keep, d_n_keep);
    SVO_HIP(hipGetLastError());
    return SVO_OK;
}

int refuse(const char *fn, const char *why, int rc)
{
    svo_set_error("%s: %s", fn, why);
    return rc;
}

}  // namespace

extern "C" {

int svo_dedup_points(svo_ctx *ctx, const float *ref_xy, int n_ref, const int *ref_idx, int n_idx, const float *new_xy, int n_new,
                     double radius, int mode, uint8_t *keep, int *n_keep, int mem)
{
    if (const char *why = check_dedup(ctx, ref_xy, n_ref, ref_idx, n_idx, new_xy, n_new, radius, mode, keep, mem))
        return refuse("svo_dedup_points", why, SVO_ERR_ARG);
    SVO_HIP(hipSetDevice(ctx->device));
    if (mem == SVO_MEM_DEVICE)
        return launch_dedup(ctx, ref_xy, n_ref, ref_idx, n_idx, new_xy, n_new, radius, mode, keep, n_keep);
    if (n_new == 0) {
        if (n_keep)
            *n_keep = 0;
        return SVO_OK;
    }
    hipStream_t st = ctx->stream;
    int rc;
    const size_t count_off = ((size_t)n_new + 63) & ~(size_t)63;   // the count lives behind the keep bytes
    if ((rc = ctx->s_a.ensure((size_t)n_ref * 8 + 8)) || (rc = ctx->s_b.ensure((size_t)n_idx * 4 + 4)) ||
        (rc = ctx->s_c.ensure((size_t)n_new * 8)) || (rc = ctx->s_g.ensure(count_off + 64)))
        return rc;
    if (n_ref)
        SVO_HIP(hipMemcpyAsync(ctx->s_a.p, ref_xy, (size_t)n_ref * 8, hipMemcpyHostToDevice, st));
    if (n_idx)
        SVO_HIP(hipMemcpyAsync(ctx->s_b.p, ref_idx, (size_t)n_idx * 4, hipMemcpyHostToDevice, st));
    SVO_HIP(hipMemcpyAsync(ctx->s_c.p, new_xy, (size_t)n_new * 8, hipMemcpyHostToDevice, st));
    uint8_t *d_keep = ctx->s_g.as<uint8_t>();
    int *d_cnt = reinterpret_cast<int *>(d_keep + count_off);
    if ((rc = launch_dedup(ctx, ctx->s_a.as<float>(), n_ref, ref_idx ? ctx->s_b.as<int>() : nullptr, n_idx, ctx->s_c.as<float>(), n_new,
                           radius, mode, d_keep, d_cnt)))
        return rc;
    SVO_HIP(hipMemcpyAsync(keep, d_keep, (size_t)n_new, hipMemcpyDeviceToHost, st));
    SVO_HIP(hipMemcpyAsync(ctx->pinned, d_cnt, sizeof(int), hipMemcpyDeviceToHost, st));
    SVO_HIP(hipStreamSynchronize(st));
    if (n_keep)
        *n_keep = *reinterpret_cast<int *>(ctx->pinned);
    return SVO_OK;
}

int svo_replenish(svo_ctx *ctx, float *ref_xy, float *ref_xyz, int n_ref, int cap, const float *new_xy, const float *new_xyz, int n_new,
                  double radius, int mode, const double *Rt, int *n_out, int *n_dup, int *n_behind, int mem)
{
    const char *why = nullptr;
    if (const int bad = check_replenish(ctx, ref_xy, ref_xyz, n_ref, cap, new_xy, new_xyz, n_new, radius, mode, Rt, mem, &why))
        return refuse("svo_replenish", why, bad == 2 ? SVO_ERR_CAPACITY : SVO_ERR_ARG);
    SVO_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const bool host = mem == SVO_MEM_HOST;
    if (host && n_new == 0) {
        if (n_out)
            *n_out = n_ref;
        if (n_dup)
            *n_dup = 0;
        if (n_behind)
            *n_behind = 0;
        return SVO_OK;
    }
    int rc;
    const size_t count_off = ((size_t)n_new + 63) & ~(size_t)63;   // host calls: three counts behind the keep bytes
    if ((rc = ctx->s_g.ensure(count_off + 64)))
        return rc;
    uint8_t *d_keep = ctx->s_g.as<uint8_t>();
    const float *d_ref = ref_xy, *d_new = new_xy, *d_xyz = new_xyz;
    float *o_xy = cap ? ref_xy + 2 * (size_t)n_ref : nullptr, *o_xyz = cap ? ref_xyz + 3 * (size_t)n_ref : nullptr;
    int *c_out = n_out, *c_dup = n_dup, *c_behind = n_behind;
    if (host) {
        if ((rc = ctx->s_a.ensure((size_t)n_ref * 8 + 8)) || (rc = ctx->s_b.ensure((size_t)n_new * 8)) ||
            (rc = ctx->s_c.ensure((size_t)n_new * 12)) || (rc = ctx->s_d.ensure((size_t)n_new * 8)) ||
            (rc = ctx->s_e.ensure((size_t)n_new * 12)))
            return rc;
        if (n_ref)
            SVO_HIP(hipMemcpyAsync(ctx->s_a.p, ref_xy, (size_t)n_ref * 8, hipMemcpyHostToDevice, st));
        SVO_HIP(hipMemcpyAsync(ctx->s_b.p, new_xy, (size_t)n_new * 8, hipMemcpyHostToDevice, st));
        SVO_HIP(hipMemcpyAsync(ctx->s_c.p, new_xyz, (size_t)n_new * 12, hipMemcpyHostToDevice, st));
        d_ref = ctx->s_a.as<float>(), d_new = ctx->s_b.as<float>(), d_xyz = ctx->s_c.as<float>();
        o_xy = ctx->s_d.as<float>(), o_xyz = ctx->s_e.as<float>();
        c_out = reinterpret_cast<int *>(d_keep + count_off), c_dup = c_out + 1, c_behind = c_out + 2;
    }
    if ((rc = launch_dedup(ctx, d_ref, n_ref, nullptr, 0, d_new, n_new, radius, mode, d_keep, nullptr)))
        return rc;
    hipLaunchKernelGGL(append_kernel, dim3(segments(n_new)), dim3(64), 0, st, to_mat34(Rt), d_keep, reinterpret_cast<const float2 *>(d_new),
                       d_xyz, n_new, segment(n_new), n_ref, reinterpret_cast<float2 *>(o_xy), o_xyz, c_out, c_dup, c_behind);
    SVO_HIP(hipGetLastError());
    if (!host)
        return SVO_OK;
    int *pin = reinterpret_cast<int *>(ctx->pinned);
    SVO_HIP(hipMemcpyAsync(pin, c_out, 3 * sizeof(int), hipMemcpyDeviceToHost, st));
    SVO_HIP(hipStreamSynchronize(st));
    const size_t k = (size_t)(pin[0] - n_ref);
    if (k) {
        SVO_HIP(hipMemcpyAsync(ref_xy + 2 * (size_t)n_ref, o_xy, k * 8, hipMemcpyDeviceToHost, st));
        SVO_HIP(hipMemcpyAsync(ref_xyz + 3 * (size_t)n_ref, o_xyz, k * 12, hipMemcpyDeviceToHost, st));
        SVO_HIP(hipStreamSynchronize(st));
    }
    if (n_out)
        *n_out = pin[0];
    if (n_dup)
        *n_dup = pin[1];
    if (n_behind)
        *n_behind = pin[2];
    return SVO_OK;
}

}  // extern "C"
