// rectify.hip -- stereo rectification and undistortion for gfx950: svo_stereo_rectify, svo_rectify_map_*, svo_remap_batch,
// svo_rectify_pairs, svo_undistort_points(_host).
//
// The definition is tests/rectify_numpy.py's (OpenCV's stereoRectify -> initUndistortRectifyMap -> remap and undistortPoints as
// recalled).  The host decisions and the per-pixel arithmetic live in rectify_plan.hip.h, which the
// kernels call, so what runs on the device is what the stand-alone check runs.
//
//   rectify_map_kernel        one thread per map pixel: (X Y W) = iR (j i 1), the camera model in double (+ - x / only), the
//                             fixed-point words.  Once per calibration.
//   rectify_map_float_kernel  the same words from a caller's float maps.
//   rectify_remap_kernel      THE HOT PATH.  One thread per four consecutive output pixels of a row: one aligned 16-byte load
//                             of the four xy words and one aligned 8-byte load of the four fractions (the map's rows are padded
//                             to a multiple of four elements), the 16 taps by plain global byte loads -- a rectifying map is
//                             smooth, neighbouring lanes hit the same lines -- and the 4 c output bytes as dword stores
//                             (shifted by a funnel when the row does not start on a dword, with byte stores at the two ends).
//                             A thread whose 16 taps all lie inside the source takes no border test; any other tests every tap.
//                             blockIdx.z: the image of the batch, or for a pair call map (z / n_pairs) and pair (z % n_pairs).
//   rectify_undistort_kernel  one thread per point, the five iterations unrolled.
// Bounds: a thread leaves unless j0 < w and i < h; it reads map elements j0 .. j0 + 3 < pitch of row i; a tap is read only after
// 0 <= x < src_w and 0 <= y < src_h were tested (the fast path tests x + 1 and y + 1 with them); it writes pixels j0 ..
// min(j0 + 4, w) - 1 of row i and no other byte.  Every offset is a size_t.
#include "svo_internal.h"
#include "rectify_plan.hip.h"

namespace rp = rectify_plan;

struct svo_rectify_map {
    int w, h, src_w, src_h, pitch;
    int device;
    char *base;            // one allocation: the xy words, then the fractions (rectify_plan::map_frac_offset)
    short *xy;             // [h][pitch][2]
    unsigned short *frac;  // [h][pitch]
};

namespace {

__global__ __launch_bounds__(256) void rectify_map_kernel(rp::MapModel m, int w, int h, int pitch, short *__restrict__ xy,
                                                          unsigned short *__restrict__ frac)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
    if (j >= pitch || i >= h)
        return;
    short2 o = make_short2(-32768, -32768);  // a pad element: outside every source
    unsigned short f = 0;
    if (j < w) {
        double u, v;
        rp::map_pixel(m, j, i, &u, &v);
        rp::map_words(u, v, &o.x, &o.y, &f);
    }
    const size_t e = (size_t)i * pitch + j;
    reinterpret_cast<short2 *>(xy)[e] = o;
    frac[e] = f;
}

__global__ __launch_bounds__(256) void rectify_map_float_kernel(const float *__restrict__ mapx, const float *__restrict__ mapy,
                                                                int w, int h, int pitch, short *__restrict__ xy,
                                                                unsigned short *__restrict__ frac)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
    if (j >= pitch || i >= h)
        return;
    short2 o = make_short2(-32768, -32768);
    unsigned short f = 0;
    if (j < w) {
        const size_t s = (size_t)i * w + j;
        rp::map_words((double)mapx[s], (double)mapy[s], &o.x, &o.y, &f);
    }
    const size_t e = (size_t)i * pitch + j;
    reinterpret_cast<short2 *>(xy)[e] = o;
    frac[e] = f;
}

struct RemapArgs {
    const short *xy[2];
    const unsigned short *frac[2];
    const uint8_t *src[2];
    uint8_t *dst[2];
    int w, h, pitch, sw, sh, per_map, value;
};

// ND dwords of packed output bytes to p, which may start anywhere in a dword
template <int ND> __device__ __forceinline__ void store_packed(uint8_t *p, const uint32_t (&v)[ND])
{
    const unsigned r = (unsigned)(reinterpret_cast<uintptr_t>(p) & 3u);
    if (r == 0) {
#pragma unroll
        for (int k = 0; k < ND; k++)
            reinterpret_cast<uint32_t *>(p)[k] = v[k];
        return;
    }
    const unsigned head = 4 - r, sh = 8 * head;  // 1..3 bytes in front of the first whole dword
#pragma unroll
    for (unsigned k = 0; k < 3; k++)
        if (k < head)
            p[k] = (uint8_t)(v[0] >> (8 * k));
    uint32_t *q = reinterpret_cast<uint32_t *>(p + head);
#pragma unroll
    for (int k = 0; k + 1 < ND; k++)
        q[k] = (v[k] >> sh) | (v[k + 1] << (32 - sh));
    uint8_t *t = p + head + 4 * (ND - 1);
    const uint32_t last = v[ND - 1] >> sh;
#pragma unroll
    for (unsigned k = 0; k < 3; k++)
        if (k < r)
            t[k] = (uint8_t)(last >> (8 * k));
}

template <int C> __global__ __launch_bounds__(rp::BLOCK_X *rp::BLOCK_Y) void rectify_remap_kernel(RemapArgs a)
{
    const int j0 = (blockIdx.x * rp::BLOCK_X + threadIdx.x) * rp::QUAD, i = blockIdx.y * rp::BLOCK_Y + threadIdx.y;
    if (j0 >= a.w || i >= a.h)
        return;
    const int m = blockIdx.z / a.per_map, k = blockIdx.z - m * a.per_map;  // uniform over the workgroup
    const size_t mo = (size_t)i * a.pitch + j0;
    // m is 0 or 1 and uniform: two selects on kernel arguments, not an indexed read of them
    const short *mxy = m ? a.xy[1] : a.xy[0];
    const unsigned short *mfrac = m ? a.frac[1] : a.frac[0];
    const int4 xy4 = *reinterpret_cast<const int4 *>(mxy + 2 * mo);
    const uint2 f2 = *reinterpret_cast<const uint2 *>(mfrac + mo);
    const uint8_t *__restrict__ src = (m ? a.src[1] : a.src[0]) + (size_t)k * a.sw * a.sh * C;
    uint8_t *dst = (m ? a.dst[1] : a.dst[0]) + ((size_t)k * a.w * a.h + (size_t)i * a.w + j0) * C;
    const int npx = min(rp::QUAD, a.w - j0);
    const int xyw[4] = {xy4.x, xy4.y, xy4.z, xy4.w};
    const unsigned fw[4] = {f2.x & 0xffffu, f2.x >> 16, f2.y & 0xffffu, f2.y >> 16};
    int x[4], y[4];
    bool fast = true;
#pragma unroll
    for (int p = 0; p < 4; p++) {
        x[p] = (short)(xyw[p] & 0xffff);
        y[p] = xyw[p] >> 16;
        fast = fast && (unsigned)x[p] < (unsigned)(a.sw - 1) && (unsigned)y[p] < (unsigned)(a.sh - 1);
    }
    uint32_t out[C];
#pragma unroll
    for (int d = 0; d < C; d++)
        out[d] = 0;
    const size_t row = (size_t)a.sw * C;
#pragma unroll
    for (int p = 0; p < 4; p++) {
        const unsigned fa = fw[p] & 31u, fb = fw[p] >> 5;
        const unsigned w00 = 32u * (32u - fa) * (32u - fb), w01 = 32u * fa * (32u - fb), w10 = 32u * (32u - fa) * fb,
                       w11 = 32u * fa * fb;
        if (fast) {
            const uint8_t *s = src + ((size_t)y[p] * a.sw + x[p]) * C;
#pragma unroll
            for (int ch = 0; ch < C; ch++) {
                const unsigned acc = w00 * s[ch] + w01 * s[C + ch] + w10 * s[row + ch] + w11 * s[row + C + ch] + (1u << 14);
                const int b = p * C + ch;
                out[b >> 2] |= (acc >> 15) << (8 * (b & 3));
            }
        } else if (p < npx) {
            const bool x0 = (unsigned)x[p] < (unsigned)a.sw, x1 = (unsigned)(x[p] + 1) < (unsigned)a.sw;
            const bool y0 = (unsigned)y[p] < (unsigned)a.sh, y1 = (unsigned)(y[p] + 1) < (unsigned)a.sh;
            const ptrdiff_t o = ((ptrdiff_t)y[p] * a.sw + x[p]) * C;  // formed, not read, unless the tap's test passed
#pragma unroll
            for (int ch = 0; ch < C; ch++) {
                const unsigned p00 = (x0 && y0) ? src[o + ch] : (unsigned)a.value;
                const unsigned p01 = (x1 && y0) ? src[o + C + ch] : (unsigned)a.value;
                const unsigned p10 = (x0 && y1) ? src[o + (ptrdiff_t)row + ch] : (unsigned)a.value;
                const unsigned p11 = (x1 && y1) ? src[o + (ptrdiff_t)row + C + ch] : (unsigned)a.value;
                const unsigned acc = w00 * p00 + w01 * p01 + w10 * p10 + w11 * p11 + (1u << 14);
                const int b = p * C + ch;
                out[b >> 2] |= (acc >> 15) << (8 * (b & 3));
            }
        }
    }
    if (npx == rp::QUAD) {
        store_packed<C>(dst, out);
    } else {  // the row's end: one to three pixels, byte by byte
#pragma unroll
        for (int b = 0; b < 3 * C; b++)
            if (b < npx * C)
                dst[b] = (uint8_t)(out[b >> 2] >> (8 * (b & 3)));
    }
}

__global__ __launch_bounds__(256) void rectify_undistort_kernel(rp::UndistortModel m, const float *__restrict__ xy, int n,
                                                                float *__restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    double x, y;
    rp::undistort_one(m, (double)xy[2 * (size_t)i], (double)xy[2 * (size_t)i + 1], &x, &y);
    out[2 * (size_t)i] = (float)x;
    out[2 * (size_t)i + 1] = (float)y;
}

int refuse(const char *fn, int kind, const char *why)
{
    svo_set_error("%s: %s", fn, why);
    return kind == 2 ? SVO_ERR_CAPACITY : SVO_ERR_ARG;
}

bool mem_ok(int mem) { return mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE; }

int map_alloc(svo_ctx *ctx, int w, int h, int src_w, int src_h, svo_rectify_map **out)
{
    svo_rectify_map *m = new svo_rectify_map();
    m->w = w, m->h = h, m->src_w = src_w, m->src_h = src_h, m->pitch = rp::map_pitch(w), m->device = ctx->device;
    void *p = nullptr;
    const hipError_t e = hipMalloc(&p, rp::map_bytes(w, h));
    if (e != hipSuccess) {
        delete m;
        svo_set_error("svo_rectify_map: hipMalloc of %zu bytes -> %s", rp::map_bytes(w, h), hipGetErrorString(e));
        return SVO_ERR_HIP;
    }
    m->base = static_cast<char *>(p);
    m->xy = reinterpret_cast<short *>(m->base);
    m->frac = reinterpret_cast<unsigned short *>(m->base + rp::map_frac_offset(w, h));
    *out = m;
    return SVO_OK;
}

// queues the remap of `images` = per_map x (1 or 2 maps) images; every pointer is a device pointer
int launch_remap(svo_ctx *ctx, const svo_rectify_map *ma, const svo_rectify_map *mb, const uint8_t *sa, const uint8_t *sb,
                 uint8_t *da, uint8_t *db, int per_map, int c, int value)
{
    RemapArgs a;
    a.xy[0] = ma->xy, a.frac[0] = ma->frac, a.src[0] = sa, a.dst[0] = da;
    a.xy[1] = mb ? mb->xy : ma->xy, a.frac[1] = mb ? mb->frac : ma->frac, a.src[1] = sb, a.dst[1] = db;
    a.w = ma->w, a.h = ma->h, a.pitch = ma->pitch, a.sw = ma->src_w, a.sh = ma->src_h, a.per_map = per_map, a.value = value;
    const rp::Grid g = rp::remap_grid(ma->w, ma->h, per_map * (mb ? 2 : 1));
    const dim3 grid(g.x, g.y, g.z), block(rp::BLOCK_X, rp::BLOCK_Y);
    if (c == 1)
        hipLaunchKernelGGL(rectify_remap_kernel<1>, grid, block, 0, ctx->stream, a);
    else
        hipLaunchKernelGGL(rectify_remap_kernel<3>, grid, block, 0, ctx->stream, a);
    SVO_HIP(hipGetLastError());
    return SVO_OK;
}

}  // namespace

extern "C" int svo_stereo_rectify(const double *K1, const double *D1, int nD1, const double *K2, const double *D2, int nD2, int w,
                                  int h, const double *R, const double *T, int flags, double alpha, int new_w, int new_h,
                                  double *R1, double *R2, double *P1, double *P2, double *Q)
{
    if (const char *why = rp::stereo_rectify(K1, D1, nD1, K2, D2, nD2, w, h, R, T, flags, alpha, new_w, new_h, R1, R2, P1, P2, Q))
        return refuse("svo_stereo_rectify", 1, why);
    return SVO_OK;
}

extern "C" int svo_undistort_points_host(const float *xy, int n, const double *K9, const double *D, int nD, const double *R9,
                                         const double *P12, double *out_xy)
{
    if (const char *why = rp::undistort_points_host(xy, n, K9, D, nD, R9, P12, out_xy))
        return refuse("svo_undistort_points_host", 1, why);
    return SVO_OK;
}

extern "C" int svo_rectify_map_create(svo_ctx *ctx, const double *K9, const double *D, int nD, const double *R9, const double *P12,
                                      int w, int h, int src_w, int src_h, svo_rectify_map **map)
{
    static const char *fn = "svo_rectify_map_create";
    if (!ctx || !map)
        return refuse(fn, 1, "ctx and map must not be null");
    rp::MapModel model;
    if (const char *why = rp::map_model(K9, D, nD, R9, P12, &model))
        return refuse(fn, 1, why);
    const char *why = nullptr;
    if (const int bad = rp::check_sizes(w, h, src_w, src_h, 1, &why))
        return refuse(fn, bad, why);
    SVO_HIP(hipSetDevice(ctx->device));
    svo_rectify_map *m = nullptr;
    if (const int rc = map_alloc(ctx, w, h, src_w, src_h, &m))
        return rc;
    hipLaunchKernelGGL(rectify_map_kernel, dim3((m->pitch + 255) / 256, h), dim3(256), 0, ctx->stream, model, w, h, m->pitch, m->xy,
                       m->frac);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess)
        e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        (void)hipFree(m->base);
        delete m;
        svo_set_error("%s: %s", fn, hipGetErrorString(e));
        return SVO_ERR_HIP;
    }
    *map = m;
    return SVO_OK;
}

extern "C" int svo_rectify_map_from_float(svo_ctx *ctx, const float *mapx, const float *mapy, int w, int h, int src_w, int src_h,
                                          int mem, svo_rectify_map **map)
{
    static const char *fn = "svo_rectify_map_from_float";
    if (!ctx || !map || !mapx || !mapy)
        return refuse(fn, 1, "ctx, mapx, mapy and map must not be null");
    if (!mem_ok(mem))
        return refuse(fn, 1, "mem must be SVO_MEM_HOST or SVO_MEM_DEVICE");
    const char *why = nullptr;
    if (const int bad = rp::check_sizes(w, h, src_w, src_h, 1, &why))
        return refuse(fn, bad, why);
    SVO_HIP(hipSetDevice(ctx->device));
    const size_t plane = (size_t)w * h * 4;
    const float *dx = mapx, *dy = mapy;
    if (mem == SVO_MEM_HOST) {
        if (const int rc = ctx->rect_stage.ensure(2 * rp::align256(plane)))
            return rc;
        char *sb = ctx->rect_stage.as<char>();
        SVO_HIP(hipMemcpyAsync(sb, mapx, plane, hipMemcpyHostToDevice, ctx->stream));
        SVO_HIP(hipMemcpyAsync(sb + rp::align256(plane), mapy, plane, hipMemcpyHostToDevice, ctx->stream));
        dx = reinterpret_cast<const float *>(sb);
        dy = reinterpret_cast<const float *>(sb + rp::align256(plane));
    }
    svo_rectify_map *m = nullptr;
    if (const int rc = map_alloc(ctx, w, h, src_w, src_h, &m))
        return rc;
    hipLaunchKernelGGL(rectify_map_float_kernel, dim3((m->pitch + 255) / 256, h), dim3(256), 0, ctx->stream, dx, dy, w, h, m->pitch,
                       m->xy, m->frac);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess)
        e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        (void)hipFree(m->base);
        delete m;
        svo_set_error("%s: %s", fn, hipGetErrorString(e));
        return SVO_ERR_HIP;
    }
    *map = m;
    return SVO_OK;
}

extern "C" int svo_rectify_map_destroy(svo_ctx *ctx, svo_rectify_map *map)
{
    if (!map)
        return SVO_OK;
    if (ctx) {
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
    }
    (void)hipFree(map->base);
    delete map;
    return SVO_OK;
}

extern "C" int svo_rectify_map_get(svo_ctx *ctx, const svo_rectify_map *map, int16_t *xy, uint16_t *frac, int mem)
{
    static const char *fn = "svo_rectify_map_get";
    if (!ctx || !map || !xy || !frac)
        return refuse(fn, 1, "ctx, map, xy and frac must not be null");
    if (!mem_ok(mem))
        return refuse(fn, 1, "mem must be SVO_MEM_HOST or SVO_MEM_DEVICE");
    SVO_HIP(hipSetDevice(ctx->device));
    const hipMemcpyKind kind = mem == SVO_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    SVO_HIP(hipMemcpy2DAsync(xy, (size_t)map->w * 4, map->xy, (size_t)map->pitch * 4, (size_t)map->w * 4, map->h, kind, ctx->stream));
    SVO_HIP(hipMemcpy2DAsync(frac, (size_t)map->w * 2, map->frac, (size_t)map->pitch * 2, (size_t)map->w * 2, map->h, kind,
                             ctx->stream));
    if (mem == SVO_MEM_HOST)
        SVO_HIP(hipStreamSynchronize(ctx->stream));
    return SVO_OK;
}

extern "C" int svo_rectify_pairs(svo_ctx *ctx, const svo_rectify_map *map_left, const svo_rectify_map *map_right,
                                 const uint8_t *lefts, const uint8_t *rights, int n_pairs, int c, int border_value,
                                 uint8_t *out_left, uint8_t *out_right, int mem)
{
    static const char *fn = "svo_rectify_pairs";
    if (!ctx || !map_left || !map_right || !lefts || !rights || !out_left || !out_right)
        return refuse(fn, 1, "ctx, both maps, both inputs and both outputs must not be null");
    if (n_pairs < 1 || n_pairs > rp::MAX_IMAGES)
        return refuse(fn, 1, "n_pairs must be 1 ... 16");
    if (c != 1 && c != 3)
        return refuse(fn, 1, "c must be 1 or 3");
    if (border_value < 0 || border_value > 255)
        return refuse(fn, 1, "border_value must be 0 ... 255");
    if (!mem_ok(mem))
        return refuse(fn, 1, "mem must be SVO_MEM_HOST or SVO_MEM_DEVICE");
    if (map_left->w != map_right->w || map_left->h != map_right->h || map_left->src_w != map_right->src_w ||
        map_left->src_h != map_right->src_h)
        return refuse(fn, 1, "the two maps must have one size and one source size");
    const char *why = nullptr;
    if (const int bad = rp::check_sizes(map_left->w, map_left->h, map_left->src_w, map_left->src_h, 2 * n_pairs, &why))
        return refuse(fn, bad, why);
    SVO_HIP(hipSetDevice(ctx->device));
    const size_t sb = (size_t)map_left->src_w * map_left->src_h * c * n_pairs, db = (size_t)map_left->w * map_left->h * c * n_pairs;
    if (mem == SVO_MEM_DEVICE)
        return launch_remap(ctx, map_left, map_right, lefts, rights, out_left, out_right, n_pairs, c, border_value);
    const size_t so = rp::align256(sb), d0 = 2 * so, d1 = d0 + rp::align256(db);
    if (const int rc = ctx->rect_stage.ensure(d1 + rp::align256(db)))
        return rc;
    uint8_t *g = ctx->rect_stage.as<uint8_t>();
    SVO_HIP(hipMemcpyAsync(g, lefts, sb, hipMemcpyHostToDevice, ctx->stream));
    SVO_HIP(hipMemcpyAsync(g + so, rights, sb, hipMemcpyHostToDevice, ctx->stream));
    if (const int rc = launch_remap(ctx, map_left, map_right, g, g + so, g + d0, g + d1, n_pairs, c, border_value))
        return rc;
    SVO_HIP(hipMemcpyAsync(out_left, g + d0, db, hipMemcpyDeviceToHost, ctx->stream));
    SVO_HIP(hipMemcpyAsync(out_right, g + d1, db, hipMemcpyDeviceToHost, ctx->stream));
    SVO_HIP(hipStreamSynchronize(ctx->stream));
    return SVO_OK;
}

extern "C" int svo_remap_batch(svo_ctx *ctx, const svo_rectify_map *map, const uint8_t *src, int n_images, int c, int border_value,
                               uint8_t *dst, int mem)
{
    static const char *fn = "svo_remap_batch";
    if (!ctx || !map || !src || !dst)
        return refuse(fn, 1, "ctx, map, src and dst must not be null");
    if (n_images < 1 || n_images > rp::MAX_IMAGES)
        return refuse(fn, 1, "n_images must be 1 ... 16");
    if (c != 1 && c != 3)
        return refuse(fn, 1, "c must be 1 or 3");
    if (border_value < 0 || border_value > 255)
        return refuse(fn, 1, "border_value must be 0 ... 255");
    if (!mem_ok(mem))
        return refuse(fn, 1, "mem must be SVO_MEM_HOST or SVO_MEM_DEVICE");
    const char *why = nullptr;
    if (const int bad = rp::check_sizes(map->w, map->h, map->src_w, map->src_h, n_images, &why))
        return refuse(fn, bad, why);
    SVO_HIP(hipSetDevice(ctx->device));
    if (mem == SVO_MEM_DEVICE)
        return launch_remap(ctx, map, nullptr, src, src, dst, dst, n_images, c, border_value);
    const size_t sb = (size_t)map->src_w * map->src_h * c * n_images, db = (size_t)map->w * map->h * c * n_images;
    const size_t d0 = rp::align256(sb);
    if (const int rc = ctx->rect_stage.ensure(d0 + rp::align256(db)))
        return rc;
    uint8_t *g = ctx->rect_stage.as<uint8_t>();
    SVO_HIP(hipMemcpyAsync(g, src, sb, hipMemcpyHostToDevice, ctx->stream));
    if (const int rc = launch_remap(ctx, map, nullptr, g, g, g + d0, g + d0, n_images, c, border_value))
        return rc;
    SVO_HIP(hipMemcpyAsync(dst, g + d0, db, hipMemcpyDeviceToHost, ctx->stream));
    SVO_HIP(hipStreamSynchronize(ctx->stream));
    return SVO_OK;
}

extern "C" int svo_undistort_points(svo_ctx *ctx, const float *xy, int n, const double *K9, const double *D, int nD,
                                    const double *R9, const double *P12, float *out_xy, int mem)
{
    static const char *fn = "svo_undistort_points";
    if (!ctx)
        return refuse(fn, 1, "ctx must not be null");
    if (n < 0)
        return refuse(fn, 1, "n must not be negative");
    if (const char *why = rp::check_camera(K9, D, nD))
        return refuse(fn, 1, why);
    if ((R9 && !rp::finite_all(R9, 9)) || (P12 && !rp::finite_all(P12, 12)))
        return refuse(fn, 1, "R and P must be finite");
    if (!mem_ok(mem))
        return refuse(fn, 1, "mem must be SVO_MEM_HOST or SVO_MEM_DEVICE");
    if (n > 0 && (!xy || !out_xy))
        return refuse(fn, 1, "xy and out_xy must not be null when n is not 0");
    if (n > rp::MAX_POINTS)
        return refuse(fn, 2, "at most 2^24 points per call");
    if (n == 0)
        return SVO_OK;
    SVO_HIP(hipSetDevice(ctx->device));
    const rp::UndistortModel model = rp::undistort_model(K9, D, nD, R9, P12);
    const size_t bytes = (size_t)n * 8;
    const float *din = xy;
    float *dout = out_xy;
    if (mem == SVO_MEM_HOST) {
        if (const int rc = ctx->rect_stage.ensure(2 * rp::align256(bytes)))
            return rc;
        char *g = ctx->rect_stage.as<char>();
        SVO_HIP(hipMemcpyAsync(g, xy, bytes, hipMemcpyHostToDevice, ctx->stream));
        din = reinterpret_cast<const float *>(g);
        dout = reinterpret_cast<float *>(g + rp::align256(bytes));
    }
    hipLaunchKernelGGL(rectify_undistort_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, model, din, n, dout);
    SVO_HIP(hipGetLastError());
    if (mem == SVO_MEM_HOST) {
        SVO_HIP(hipMemcpyAsync(out_xy, dout, bytes, hipMemcpyDeviceToHost, ctx->stream));
        SVO_HIP(hipStreamSynchronize(ctx->stream));
    }
    return SVO_OK;
}
