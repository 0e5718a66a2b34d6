// feature_batch.hip.h -- the host plumbing the feature modules share (sift.hip, brief.hip, surf.hip): a batch of images of one size
// in, per-image counts and columns of per-key-point values out.  Each module includes it inside its own unnamed namespace, after
// svo_internal.h.  Everything runs on the context's one stream, so the staging buffers (svo_ctx::feat_img, ::feat_sum) are never
// live for two calls at once.
#pragma once

// the images of one launch, a kernel argument: blockIdx.y or .z picks the image.  The public limit of every batched entry point.
constexpr int IMAGE_MAXBATCH = 16;
struct ImageBatch {
    const uint8_t *img[IMAGE_MAXBATCH];
};
static_assert(IMAGE_MAXBATCH == 16 && sizeof(ImageBatch) == 16 * sizeof(const uint8_t *),
              "svo.h promises 1 ... 16 images per call; the kernels take the table as it is");

inline ImageBatch make_image_batch(const uint8_t *const *d_images, int nb)
{
    ImageBatch im;
    for (int k = 0; k < IMAGE_MAXBATCH; k++)
        im.img[k] = k < nb ? d_images[k] : nullptr;
    return im;
}

inline bool aligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

// the next `count` elements of a work buffer; every array starts on a 256-byte boundary
template <class T> T *bump(uint8_t *&p, size_t count)
{
    T *r = reinterpret_cast<T *>(p);
    p += (count * sizeof(T) + 255) & ~(size_t)255;
    return r;
}

// the device addresses of a call's nb images: host images are copied into 256-byte-aligned, evenly spaced slots of ctx->feat_img
// (surf.hip uses staged grey images in place through image 0's address and that stride), device images are used where they are
inline int stage_images(svo_ctx *ctx, const uint8_t *const *images, int nb, size_t img_bytes, int mem, const uint8_t **ptrs)
{
    if (mem != SVO_MEM_HOST) {
        for (int k = 0; k < nb; k++)
            ptrs[k] = images[k];
        return SVO_OK;
    }
    const size_t slot = (img_bytes + 255) & ~(size_t)255;
    int rc;
    if ((rc = ctx->feat_img.ensure(slot * nb + 256)))
        return rc;
    for (int k = 0; k < nb; k++) {
        uint8_t *dst = ctx->feat_img.as<uint8_t>() + (size_t)k * slot;
        SVO_HIP(hipMemcpyAsync(dst, images[k], img_bytes, hipMemcpyHostToDevice, ctx->stream));
        ptrs[k] = dst;
    }
    return SVO_OK;
}

// the one wait of an extract call: n counts from the device
inline int read_counts(svo_ctx *ctx, const int *d_counts, int n, int *host_counts)
{
    SVO_HIP(hipMemcpyAsync(host_counts, d_counts, sizeof(int) * n, hipMemcpyDeviceToHost, ctx->stream));
    SVO_HIP(hipStreamSynchronize(ctx->stream));
    return SVO_OK;
}

// one output column of a host call: n_images x cap entries of `bytes` bytes on both sides; a null host pointer = not asked for
struct HostColumn {
    void *host;
    const void *dev;
    size_t bytes;
};

// the first min(n[k], cap) rows of every column of every image, then the wait for them
inline int copy_rows_to_host(hipStream_t st, const HostColumn *cols, int n_cols, int n_images, int cap, const int *n)
{
    for (int k = 0; k < n_images; k++) {
        const size_t m = (size_t)(n[k] < cap ? n[k] : cap), b = (size_t)k * cap;
        if (!m)
            continue;
        for (int c = 0; c < n_cols; c++)
            if (cols[c].host)
                SVO_HIP(hipMemcpyAsync(static_cast<uint8_t *>(cols[c].host) + b * cols[c].bytes,
                                       static_cast<const uint8_t *>(cols[c].dev) + b * cols[c].bytes, m * cols[c].bytes,
                                       hipMemcpyDeviceToHost, st));
    }
    SVO_HIP(hipStreamSynchronize(st));
    return SVO_OK;
}
