// scan_selftest.hip -- svo_selftest_scan: scan_ops.hip.h's block_scan_counts in a single workgroup, so that a test can hold the
// header every compaction stands on against a cumulative sum at the lane, wave, workgroup and chunk seams.
#include "svo_internal.h"
#include "scan_ops.hip.h"

namespace {

template <int THREADS, class T>
__global__ __launch_bounds__(THREADS) void selftest_scan_kernel(const T *in, T *out, int n, T *total)   // out == in is allowed
{
    __shared__ T s_wave[THREADS / 64];
    const T all = svo::block_scan_counts<THREADS>(in, out, n, s_wave);
    if (threadIdx.x == 0)
        *total = all;
}

template <int THREADS, class T> void launch(hipStream_t st, const void *d_in, int n, void *d_out, void *d_total)
{
    hipLaunchKernelGGL((selftest_scan_kernel<THREADS, T>), dim3(1), dim3(THREADS), 0, st, static_cast<const T *>(d_in), static_cast<T *>(d_out),
                       n, static_cast<T *>(d_total));
}

}  // namespace

extern "C" int svo_selftest_scan(svo_ctx *ctx, int kind, const void *d_in, int n, void *d_out, void *d_total)
{
    SVO_CHECK_ARG(ctx && n >= 0 && n <= (1 << 24) && d_total && (n == 0 || (d_in && d_out)));
    SVO_CHECK_ARG(kind >= SVO_SCAN_256_INT && kind <= SVO_SCAN_1024_U64);
    SVO_HIP(hipSetDevice(ctx->device));
    if (kind == SVO_SCAN_256_INT)
        launch<256, int>(ctx->stream, d_in, n, d_out, d_total);
    else if (kind == SVO_SCAN_1024_UINT)
        launch<1024, unsigned>(ctx->stream, d_in, n, d_out, d_total);
    else
        launch<1024, unsigned long long>(ctx->stream, d_in, n, d_out, d_total);
    SVO_HIP(hipGetLastError());
    SVO_HIP(hipStreamSynchronize(ctx->stream));
    return SVO_OK;
}
