// N5 sparse trainer: torch.optim.SparseAdam's update over the rows of a batch (mi_lazy_adam_rows_f32; include/laplace_hip.h,
// additive to ABI 14).  The chain of one row is lazy_adam.hpp's; here it runs over n distinct row ids with their gradient rows
// given compactly — the id-only PinSAGE model's path: the executor hands back the gradient of blocks[0].src_ids' rows through
// rows_out, those ids are distinct, so neither a sort nor a table-sized gradient buffer is needed.  One lane per float4 of a
// row; a call reads and writes 7 * n * width * 4 bytes whatever the table's size.
#include "lazy_adam.hpp"

namespace {

constexpr int kBlock = 256;

__global__ __launch_bounds__(kBlock) void lazy_adam_rows_kernel(int64_t n, int w4, const int64_t* __restrict__ ids,
                                                                const float4* __restrict__ g, int64_t ldg4, float4* __restrict__ p,
                                                                float4* __restrict__ m, float4* __restrict__ v, MiLazyConsts c) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n * w4) return;
    const int64_t r = i / w4;
    const int e = (int)(i - r * w4);
    const int64_t off = ids[r] * w4 + e;
    float4 pp = p[off], mm = m[off], vv = v[off];
    mi_lazy_adam_update4(pp, g[r * ldg4 + e], mm, vv, c);
    p[off] = pp;
    m[off] = mm;
    v[off] = vv;
}

}  // namespace

extern "C" {

int64_t mi_lazy_adam_sizeof(int32_t which) {
    switch (which) {
        case 0: return (int64_t)sizeof(mi_lazy_adam);
        case 1: return (int64_t)sizeof(mi_item_projector_moments);
        default: return -1;
    }
}

int mi_lazy_adam_rows_f32(int64_t rows, int32_t width, float* p, float* m, float* v, int64_t n, const int64_t* ids, const float* g,
                          int64_t ldg, const mi_lazy_adam* lazy, mi_stream_t stream) {
    const int bad = mi_lazy_check(lazy);
    if (bad) return bad;
    if (width < 4 || width % 4 != 0 || width > 512) return MI_ERR_UNSUPPORTED;
    MI_CHECK_ARG(rows >= 1 && n >= 0 && n <= rows);
    MI_CHECK_ARG(p && m && v && mi_aligned16(p) && mi_aligned16(m) && mi_aligned16(v));
    if (rows >= ((int64_t)1 << 40)) return MI_ERR_TOO_LARGE;
    if (n == 0) return 0;
    MI_CHECK_ARG(ids && (reinterpret_cast<uintptr_t>(ids) & 7u) == 0 && g && mi_aligned16(g) && ldg >= width && ldg % 4 == 0);
    const int w4 = width / 4;
    if (n * (int64_t)w4 >= ((int64_t)INT32_MAX) * kBlock) return MI_ERR_TOO_LARGE;
    // ---- nothing has been enqueued up to here ----
    hipLaunchKernelGGL(lazy_adam_rows_kernel, dim3((unsigned)mi_ceil_div(n * w4, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, n, w4,
                       ids, reinterpret_cast<const float4*>(g), ldg / 4, reinterpret_cast<float4*>(p), reinterpret_cast<float4*>(m),
                       reinterpret_cast<float4*>(v), mi_lazy_consts(*lazy));
    return mi_launch_status();
}

}  // extern "C"
