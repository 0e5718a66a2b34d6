// integral_scan.hip.h -- the batched int32 integral image of 8-bit images (grey, or BGR through svo_bgr2gray): (h + 1) x (w + 1),
// zero first row and column; blockIdx.y = image of the batch.  Shared by brief.hip and surf.hip; each includes it inside its own
// unnamed namespace, after feature_batch.hip.h, and includes scan_ops.hip.h (the row scan's block scan) at file scope before that.
// Integer sums: exact, no order dependence.
#pragma once

// the largest entry is at most 255 w h
inline bool integral_fits_int32(int w, int h) { return 255ll * w * h <= 2147483647ll; }

// ints between the tables of two images of a batch
inline long long integral_img_stride(int w, int h) { return (((long long)(w + 1) * (h + 1)) + 63) & ~63ll; }

// row y of the image -> row y + 1 of the table, as running sums along the row; column 0 and row 0 are zero
__global__ __launch_bounds__(256) void integral_row_scan_kernel(ImageBatch im, int w, int h, int c, int *__restrict__ sum_all,
                                                             long long img_stride)
{
    __shared__ int s_wave[4];
    const int y = blockIdx.x;
    const uint8_t *__restrict__ row = im.img[blockIdx.y] + (size_t)y * w * c;
    int *__restrict__ out = sum_all + blockIdx.y * img_stride + (size_t)(y + 1) * (w + 1);
    if (threadIdx.x == 0)
        out[0] = 0;
    if (y == 0)
        for (int x = threadIdx.x; x <= w; x += 256)
            out[x - (w + 1)] = 0;
    int carry = 0;
    for (int x0 = 0; x0 < w; x0 += 256) {
        const int x = x0 + threadIdx.x;
        int v = 0;
        if (x < w)
            v = c == 1 ? (int)row[x] : svo_bgr2gray(row[3 * x], row[3 * x + 1], row[3 * x + 2]);
        int all;
        const int before = svo::block_excl_scan<256>(v, s_wave, &all);
        if (x < w)
            out[x + 1] = carry + before + v;   // the inclusive sum
        carry += all;
        __syncthreads();
    }
}

// a thread per column 1 ... w: rows added up from the top; eight rows' loads are in flight before the first add
__global__ __launch_bounds__(64) void integral_col_scan_kernel(int w, int h, int *__restrict__ sum_all, long long img_stride)
{
    const int x = blockIdx.x * 64 + threadIdx.x + 1;
    if (x > w)
        return;
    const size_t pitch = (size_t)w + 1;
    int *__restrict__ p = sum_all + blockIdx.y * img_stride + pitch + x;
    int acc = 0, y = 0;
    for (; y + 8 <= h; y += 8) {
        int v[8];
#pragma unroll
        for (int k = 0; k < 8; k++)
            v[k] = p[(size_t)(y + k) * pitch];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            acc += v[k];
            p[(size_t)(y + k) * pitch] = acc;
        }
    }
    for (; y < h; y++) {
        acc += p[(size_t)y * pitch];
        p[(size_t)y * pitch] = acc;
    }
}

// the integral images of nb device images into ctx->feat_sum, which also gets room for extra_bytes behind them
inline int integral_images(svo_ctx *ctx, const uint8_t *const *d_images, int nb, int w, int h, int c, size_t extra_bytes)
{
    const long long stride = integral_img_stride(w, h);
    int rc;
    if ((rc = ctx->feat_sum.ensure((size_t)stride * nb * 4 + extra_bytes)))
        return rc;
    hipLaunchKernelGGL(integral_row_scan_kernel, dim3(h, nb), dim3(256), 0, ctx->stream, make_image_batch(d_images, nb), w, h, c,
                       ctx->feat_sum.as<int>(), stride);
    hipLaunchKernelGGL(integral_col_scan_kernel, dim3((w + 63) / 64, nb), dim3(64), 0, ctx->stream, w, h, ctx->feat_sum.as<int>(),
                       stride);
    SVO_HIP(hipGetLastError());
    return SVO_OK;
}
