// voxel.hip -- voxel-grid down-sampling of a cloud of up to 2^22 points for gfx950: svo_voxel_downsample, svo_voxel_grid.
//
// The definition is tests/voxel_numpy.py's (Open3D's VoxelDownSample as recalled): points with a
// non-finite coordinate dropped, min_bound = min - leaf / 2 over the rest, the cell of a coordinate floor((p - min_bound) / leaf)
// in double, one output row per occupied cell in ascending (z, y, x) cell order, every component the double sum of the cell's
// points in ascending input index divided by the count and rounded to float at the store.
//
//   1. voxel_bounds_kernel / voxel_bounds_final_kernel: min, max and count of the finite points (exact, so any order serves).
//      The host reads them, forms the grid (voxel_plan::grid) and refuses a cloud that spans 2^21 cells or more on an axis
//      before any key is formed.
//   2. voxel_key_kernel: the packed cell of every point; a dropped point gets the largest key (cloud_index.hip.h's convention).
//   3. radix_sort_pairs of (key, index): stable, so a cell's points stand in ascending input index afterwards -- the order
//      the definition sums in.
//   4. voxel_head_count_kernel, voxel_scan_blocks_kernel, voxel_rows_kernel: a sorted position whose key differs from its
//      predecessor's heads a voxel; the scan of the heads (scan_ops.hip.h) is the output row of every position.  The last also
//      gathers the points (and colours) into voxel order through the sorted index, writes the segment starts and scatters
//      the trace (point_voxel).
//   5. voxel_mean_kernel: ONE WAVE PER VOXEL.  The wave loads 64 consecutive gathered rows at a time (contiguous floats:
//      coalesced) into its LDS slice, then lane c runs the chain of component c over them: a dependent double add per point
//      whose operand comes from LDS, not from HBM.  The chain is serial by definition; a cloud that falls into one voxel costs
//      one dependent add per point on a single wave (DESIGN.md section 10o has the measured cost).
// Every loop is bounded by the counts the host passed (n, m) or by a segment's two ends, which the rows kernel wrote inside
// [0, m]; every index formed fits 32 bits (n <= 2^22, 6 n < 2^25).
#include "svo_internal.h"
#include "cloud_index.hip.h"
#include "voxel_plan.hip.h"

namespace vp = voxel_plan;
static_assert(vp::TILE == RS_TILE && vp::BLOCK == RS_THREADS, "the tiles of voxel.hip are the radix sort's");

namespace {

struct VoxelGrid {
    double min_bound[3];
    double leaf;
};

__device__ __forceinline__ bool finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// part[8 b ..]: lo x y z, hi x y z, the finite count (int bits), pad -- of tile b
__global__ __launch_bounds__(vp::BLOCK) void voxel_bounds_kernel(const float *__restrict__ xyz, int n, float *__restrict__ part)
{
    __shared__ float s_lo[4][3], s_hi[4][3];
    __shared__ int s_cnt[4];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()};
    float hi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    int cnt = 0;
    const int base = blockIdx.x * vp::TILE;
    for (int r = 0; r < vp::TILE / vp::BLOCK; r++) {
        const int i = base + r * vp::BLOCK + tid;
        if (i < n) {
            const float p[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
            if (finite3(p[0], p[1], p[2])) {
                cnt++;
#pragma unroll
                for (int a = 0; a < 3; a++) {
                    lo[a] = fminf(lo[a], p[a]);
                    hi[a] = fmaxf(hi[a], p[a]);
                }
            }
        }
    }
#pragma unroll
    for (int a = 0; a < 3; a++) {
        lo[a] = svo::wave_min(lo[a]);
        hi[a] = svo::wave_max(hi[a]);
    }
    cnt = svo::wave_sum_dpp(cnt);
    if (lane == 0) {
#pragma unroll
        for (int a = 0; a < 3; a++) {
            s_lo[w][a] = lo[a];
            s_hi[w][a] = hi[a];
        }
        s_cnt[w] = cnt;
    }
    __syncthreads();
    if (tid < 3) {
        part[8 * blockIdx.x + tid] = fminf(fminf(s_lo[0][tid], s_lo[1][tid]), fminf(s_lo[2][tid], s_lo[3][tid]));
        part[8 * blockIdx.x + 3 + tid] = fmaxf(fmaxf(s_hi[0][tid], s_hi[1][tid]), fmaxf(s_hi[2][tid], s_hi[3][tid]));
    } else if (tid == 3) {
        part[8 * blockIdx.x + 6] = __int_as_float(s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3]);
        part[8 * blockIdx.x + 7] = 0.f;
    }
}

// one workgroup of 1024: the nblk <= 1024 tile records -> out[0..7], the same record for the cloud
__global__ __launch_bounds__(1024) void voxel_bounds_final_kernel(const float *__restrict__ part, int nblk, float *__restrict__ out)
{
    __shared__ float s_lo[16][3], s_hi[16][3];
    __shared__ int s_cnt[16];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()};
    float hi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    int cnt = 0;
    for (int b = tid; b < nblk; b += 1024) {
#pragma unroll
        for (int a = 0; a < 3; a++) {
            lo[a] = fminf(lo[a], part[8 * b + a]);
            hi[a] = fmaxf(hi[a], part[8 * b + 3 + a]);
        }
        cnt += __float_as_int(part[8 * b + 6]);
    }
#pragma unroll
    for (int a = 0; a < 3; a++) {
        lo[a] = svo::wave_min(lo[a]);
        hi[a] = svo::wave_max(hi[a]);
    }
    cnt = svo::wave_sum_dpp(cnt);
    if (lane == 0) {
#pragma unroll
        for (int a = 0; a < 3; a++) {
            s_lo[w][a] = lo[a];
            s_hi[w][a] = hi[a];
        }
        s_cnt[w] = cnt;
    }
    __syncthreads();
    if (tid < 3) {
        float l = s_lo[0][tid], h = s_hi[0][tid];
        for (int q = 1; q < 16; q++) {
            l = fminf(l, s_lo[q][tid]);
            h = fmaxf(h, s_hi[q][tid]);
        }
        out[tid] = l;
        out[3 + tid] = h;
    } else if (tid == 3) {
        int c = 0;
        for (int q = 0; q < 16; q++)
            c += s_cnt[q];
        out[6] = __int_as_float(c);
        out[7] = 0.f;
    }
}

__global__ __launch_bounds__(vp::BLOCK) void voxel_key_kernel(const float *__restrict__ xyz, int n, VoxelGrid g,
                                                              uint64_t *__restrict__ keys, int *__restrict__ vals)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    uint64_t key = vp::DROPPED_KEY;
    if (finite3(x, y, z))
        key = vp::pack_key(vp::cell_index(x, g.min_bound[0], g.leaf), vp::cell_index(y, g.min_bound[1], g.leaf),
                           vp::cell_index(z, g.min_bound[2], g.leaf));
    keys[i] = key;
    vals[i] = i;
}

// sorted position i (of the m finite points) heads a voxel when its key differs from its predecessor's
__device__ __forceinline__ bool voxel_head(const uint64_t *__restrict__ keys, int i, int m)
{
    return i < m && (i == 0 || keys[i] != keys[i - 1]);
}

__global__ __launch_bounds__(vp::BLOCK) void voxel_head_count_kernel(const uint64_t *__restrict__ keys, int m,
                                                                     int *__restrict__ blk)
{
    __shared__ int s_cnt[4];
    const int tid = threadIdx.x;
    const int base = blockIdx.x * vp::TILE;
    int cnt = 0;
    for (int r = 0; r < vp::TILE / vp::BLOCK; r++)
        cnt += voxel_head(keys, base + r * vp::BLOCK + tid, m) ? 1 : 0;
    int total;
    svo::waves_before<vp::BLOCK>(svo::wave_sum_dpp(cnt), s_cnt, &total);
    if (tid == 0)
        blk[blockIdx.x] = total;
}

// exclusive scan of the nblk <= 1024 tile counts in place, one workgroup; *n_out = their total
__global__ __launch_bounds__(1024) void voxel_scan_blocks_kernel(int *__restrict__ blk, int nblk, int *__restrict__ n_out)
{
    __shared__ int s_wave[16];
    const int total = svo::block_scan_counts<1024>(blk, blk, nblk, s_wave);   // one chunk
    if (threadIdx.x == 0)
        *n_out = total;
}

// Every sorted position's output row (the inclusive scan of the heads, minus one), in tile order as the radix scatter ranks:
// lane order inside a wave by ballot, wave order inside a round, round order inside the tile.  Writes seg[row] = the position a
// voxel starts at and seg[n_out] = m, gathers the point (and colour) of position i into rows[i c ..] and scatters the trace.
__global__ __launch_bounds__(vp::BLOCK) void voxel_rows_kernel(const uint64_t *__restrict__ keys, const int *__restrict__ vals,
                                                               int n, int m, const int *__restrict__ blk,
                                                               const float *__restrict__ xyz, const float *__restrict__ color,
                                                               float *__restrict__ rows, int *__restrict__ seg,
                                                               int *__restrict__ point_voxel)
{
    __shared__ int s_w[4];
    const int tid = threadIdx.x;
    const int c = color ? 6 : 3;
    const int base = blockIdx.x * vp::TILE;
    int run = blk[blockIdx.x];
    for (int r = 0; r < vp::TILE / vp::BLOCK && base + r * vp::BLOCK < n; r++) {  // the bound is uniform over the workgroup
        const int i = base + r * vp::BLOCK + tid;
        const bool head = voxel_head(keys, i, m);
        const unsigned long long bal = __ballot(head);
        int total;
        const int before = svo::waves_before<vp::BLOCK>((int)__popcll(bal), s_w, &total);
        // heads up to and INCLUDING i, minus one: the inclusive count is the lanes below plus the lane's own bit
        const int row = run + before + svo::lanes_below(bal) + (head ? 1 : 0) - 1;
        if (i < n) {
            const int j = vals[i];
            if (i < m) {
                if (head)
                    seg[row] = i;
                if (i == m - 1)
                    seg[row + 1] = m;
                rows[(size_t)i * c] = xyz[3 * j];
                rows[(size_t)i * c + 1] = xyz[3 * j + 1];
                rows[(size_t)i * c + 2] = xyz[3 * j + 2];
                if (color) {
                    rows[(size_t)i * c + 3] = color[3 * j];
                    rows[(size_t)i * c + 4] = color[3 * j + 1];
                    rows[(size_t)i * c + 5] = color[3 * j + 2];
                }
            }
            if (point_voxel)
                point_voxel[j] = i < m ? row : -1;
        }
        __syncthreads();
        run += total;
    }
}

__global__ __launch_bounds__(vp::BLOCK) void voxel_fill_kernel(int *__restrict__ p, int n, int v)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        p[i] = v;
}

// one wave per voxel; c = 3 or 6 floats a gathered row
__global__ __launch_bounds__(64 * vp::MEAN_WAVES) void voxel_mean_kernel(const float *__restrict__ rows,
                                                                         const int *__restrict__ seg,
                                                                         const int *__restrict__ d_n_out, int c,
                                                                         float *__restrict__ xyz_out, float *__restrict__ color_out,
                                                                         int *__restrict__ voxel_count)
{
    __shared__ float s_rows[vp::MEAN_WAVES][64 * 6];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int v = __builtin_amdgcn_readfirstlane(blockIdx.x * vp::MEAN_WAVES + w);
    if (v >= *d_n_out)
        return;
    float *buf = s_rows[w];
    const int s = seg[v], e = seg[v + 1];
    double sum = 0.0;
    for (int base = s; base < e; base += 64) {
        const int cnt = min(64, e - base);
        const float *src = rows + (size_t)base * c;
        for (int t = lane; t < cnt * c; t += 64)
            buf[t] = src[t];
        svo::wave_lds_fence();
        if (lane < c)
            for (int k = 0; k < cnt; k++)
                sum += (double)buf[k * c + lane];  // left to right: ascending input index
        svo::wave_lds_fence();
    }
    if (lane < c) {
        const float mean = (float)(sum / (double)(e - s));
        if (lane < 3)
            xyz_out[3 * v + lane] = mean;
        else
            color_out[3 * v + lane - 3] = mean;
    }
    if (lane == 0 && voxel_count)
        voxel_count[v] = e - s;
}

}  // namespace

extern "C" int svo_voxel_grid(const float *min_xyz, const float *max_xyz, double voxel_size, double *min_bound3, int64_t *cells3)
{
    const char *why = nullptr;
    const int rc = vp::grid(min_xyz, max_xyz, voxel_size, min_bound3, cells3, &why);
    if (rc)
        svo_set_error("svo_voxel_grid: %s", why);
    return rc == 0 ? SVO_OK : (rc == 1 ? SVO_ERR_ARG : SVO_ERR_CAPACITY);
}

extern "C" int svo_voxel_downsample(svo_ctx *ctx, const float *xyz, const float *color, int n, double voxel_size, float *xyz_out,
                                    float *color_out, int *n_out, int *point_voxel, int *voxel_count, int mem)
{
    if (const char *why = vp::check_args(ctx, xyz, color, n, voxel_size, xyz_out, color_out, n_out, mem)) {
        svo_set_error("svo_voxel_downsample: %s", why);
        return SVO_ERR_ARG;
    }
    if (n > vp::MAX_POINTS) {
        svo_set_error("svo_voxel_downsample: %d points, at most %d per call", n, vp::MAX_POINTS);
        return SVO_ERR_CAPACITY;
    }
    if (n == 0) {
        if (n_out)
            *n_out = 0;
        return SVO_OK;
    }
    const int c = color ? 6 : 3;
    const vp::Layout L = vp::layout(n, c);
    int rc;
    if ((rc = ctx->voxel_work.ensure(L.total)))
        return rc;
    char *g = ctx->voxel_work.as<char>();
    uint64_t *k0 = reinterpret_cast<uint64_t *>(g + L.k0), *k1 = reinterpret_cast<uint64_t *>(g + L.k1);
    int *v0 = reinterpret_cast<int *>(g + L.v0), *v1 = reinterpret_cast<int *>(g + L.v1);
    unsigned *hist = reinterpret_cast<unsigned *>(g + L.hist);
    float *rows = reinterpret_cast<float *>(g + L.rows), *part = reinterpret_cast<float *>(g + L.part);
    int *seg = reinterpret_cast<int *>(g + L.seg), *blk = reinterpret_cast<int *>(g + L.blk);
    float *scal = reinterpret_cast<float *>(g + L.scal);
    int *d_n_out = reinterpret_cast<int *>(g + L.scal) + 8;
    hipStream_t st = ctx->stream;

    const float *dx = xyz, *dc = color;
    float *ox = xyz_out, *oc = color_out;
    int *opv = point_voxel, *ovc = voxel_count;
    if (mem == SVO_MEM_HOST) {
        const vp::Stage S = vp::stage(n);
        if ((rc = ctx->voxel_stage.ensure(S.total)))
            return rc;
        char *sb = ctx->voxel_stage.as<char>();
        SVO_HIP(hipMemcpyAsync(sb + S.xyz, xyz, (size_t)n * 12, hipMemcpyHostToDevice, st));
        if (color)
            SVO_HIP(hipMemcpyAsync(sb + S.color, color, (size_t)n * 12, hipMemcpyHostToDevice, st));
        dx = reinterpret_cast<const float *>(sb + S.xyz);
        dc = color ? reinterpret_cast<const float *>(sb + S.color) : nullptr;
        ox = reinterpret_cast<float *>(sb + S.xyz_out);
        oc = reinterpret_cast<float *>(sb + S.color_out);
        opv = point_voxel ? reinterpret_cast<int *>(sb + S.point_voxel) : nullptr;
        ovc = voxel_count ? reinterpret_cast<int *>(sb + S.voxel_count) : nullptr;
    }

    // 1. the finite bounds; the grid and the refusal are the host's
    const int nblk = vp::tiles(n);
    const dim3 b256(vp::BLOCK), g256((n + vp::BLOCK - 1) / vp::BLOCK);
    hipLaunchKernelGGL(voxel_bounds_kernel, dim3(nblk), b256, 0, st, dx, n, part);
    hipLaunchKernelGGL(voxel_bounds_final_kernel, dim3(1), dim3(1024), 0, st, part, nblk, scal);
    SVO_HIP(hipGetLastError());
    SVO_HIP(hipMemcpyAsync(ctx->pinned, scal, 32, hipMemcpyDeviceToHost, st));
    SVO_HIP(hipStreamSynchronize(st));
    float bounds[8];
    std::memcpy(bounds, ctx->pinned, 32);
    int m;
    std::memcpy(&m, &bounds[6], 4);
    if (m <= 0) {  // every point is non-finite: no voxel, every point dropped
        if (opv)
            hipLaunchKernelGGL(voxel_fill_kernel, g256, b256, 0, st, opv, n, -1);
        SVO_HIP(hipGetLastError());
        if (mem == SVO_MEM_HOST && point_voxel)
            SVO_HIP(hipMemcpyAsync(point_voxel, opv, (size_t)n * 4, hipMemcpyDeviceToHost, st));
        SVO_HIP(hipStreamSynchronize(st));
        *n_out = 0;
        return SVO_OK;
    }
    VoxelGrid grid;
    int64_t cells[3];
    const char *why = nullptr;
    if (const int bad = vp::grid(bounds, bounds + 3, voxel_size, grid.min_bound, cells, &why)) {
        svo_set_error("svo_voxel_downsample: %s", why);
        return bad == 1 ? SVO_ERR_ARG : SVO_ERR_CAPACITY;
    }
    grid.leaf = voxel_size;

    // 2. - 5.
    hipLaunchKernelGGL(voxel_key_kernel, g256, b256, 0, st, dx, n, grid, k0, v0);
    if ((rc = radix_sort_pairs(st, k0, v0, k1, v1, n, hist)))
        return rc;
    hipLaunchKernelGGL(voxel_head_count_kernel, dim3(nblk), b256, 0, st, k0, m, blk);
    hipLaunchKernelGGL(voxel_scan_blocks_kernel, dim3(1), dim3(1024), 0, st, blk, nblk, d_n_out);
    hipLaunchKernelGGL(voxel_rows_kernel, dim3(nblk), b256, 0, st, k0, v0, n, m, blk, dx, dc, rows, seg, opv);
    hipLaunchKernelGGL(voxel_mean_kernel, dim3(vp::mean_blocks(m)), dim3(64 * vp::MEAN_WAVES), 0, st, rows, seg, d_n_out, c, ox,
                       oc, ovc);
    SVO_HIP(hipGetLastError());
    SVO_HIP(hipMemcpyAsync(ctx->pinned, d_n_out, 4, hipMemcpyDeviceToHost, st));
    SVO_HIP(hipStreamSynchronize(st));
    const int rows_out = *reinterpret_cast<int *>(ctx->pinned);
    if (mem == SVO_MEM_HOST) {
        SVO_HIP(hipMemcpyAsync(xyz_out, ox, (size_t)rows_out * 12, hipMemcpyDeviceToHost, st));
        if (color)
            SVO_HIP(hipMemcpyAsync(color_out, oc, (size_t)rows_out * 12, hipMemcpyDeviceToHost, st));
        if (point_voxel)
            SVO_HIP(hipMemcpyAsync(point_voxel, opv, (size_t)n * 4, hipMemcpyDeviceToHost, st));
        if (voxel_count)
            SVO_HIP(hipMemcpyAsync(voxel_count, ovc, (size_t)rows_out * 4, hipMemcpyDeviceToHost, st));
        SVO_HIP(hipStreamSynchronize(st));
    }
    *n_out = rows_out;
    return SVO_OK;
}
