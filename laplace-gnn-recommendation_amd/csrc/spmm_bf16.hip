// bf16 layer tables of the LightGCN forward (include/laplace_hip.h, "bf16 layer tables"): the CSR product with a bf16 operand
// and f32 values, sums and epilogue; the f32 -> bf16 image of a table; the bf16 -> f32 row gather of the batch's layer sum.
//
// The product follows spmm.hip's plain forms and none of its variants: a short row is one sub-group's fma chain in list
// order, a split row is one such chain per work item of the plan (partial f32 rows in the workspace) and a fix-up that adds
// the partial rows in a fixed order.  No float atomics, equal bits from run to run, and the row-list form runs the same
// chains as the dense form.  What changes is the gathered row: 2 bytes per element, so a lane's one 16-byte load is 8
// elements, a row of d = 128 is 16 lanes, and one wave-instruction fetches four neighbour rows of 256 bytes.
#include "common.hpp"

namespace {

constexpr int kWavesPerBlock = 4;
constexpr int kBlock = kWavesPerBlock * MI_WAVE;
constexpr int kPlanGroup = MI_SPMM_GROUP;
constexpr int kUnroll = 4;        // row loads in flight per lane before the first fma, as in spmm_rows_kernel
constexpr int kFixupUnroll = 8;   // partial rows in flight per lane of the fix-up

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

// two f32 -> one dword of two bf16, round to nearest even: the compiler selects the packed conversion of gfx950
__device__ __forceinline__ uint32_t pack2(float lo, float hi) {
    f32x2 f = {lo, hi};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(f, bf16x2));
}
__device__ __forceinline__ float bf16_lo(uint32_t w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bf16_hi(uint32_t w) { return __uint_as_float(w & 0xFFFF0000u); }

__device__ __forceinline__ uint2 pack4(const float4& a) { return make_uint2(pack2(a.x, a.y), pack2(a.z, a.w)); }
__device__ __forceinline__ float4 unpack4(const uint2& b) {
    return make_float4(bf16_lo(b.x), bf16_hi(b.x), bf16_lo(b.y), bf16_hi(b.y));
}

struct Out {
    uint16_t* Y;          int64_t ldy;    // bf16 rows, ld in elements
    const float4* addend; int64_t lda4;
    float4* S;            int64_t lds4;
    float scale;
};

// Columns [4 e4, 4 e4 + 4) of output row r: S = scale * (addend + (Y ? float(rn(acc)) : acc)); returns rn(acc) for the caller's
// Y store (the short-row kernel stores two of them as one 16-byte row piece).
__device__ __forceinline__ uint2 finish4(const Out& ep, int64_t r, int e4, const float4& acc) {
    const uint2 yb = pack4(acc);
    if (ep.S) {
        const float4 v = ep.Y ? unpack4(yb) : acc;
        const float4 a = ep.addend ? ep.addend[r * ep.lda4 + e4] : mi_f4_zero();
        float4 o;
        o.x = ep.scale * (a.x + v.x);
        o.y = ep.scale * (a.y + v.y);
        o.z = ep.scale * (a.z + v.z);
        o.w = ep.scale * (a.w + v.w);
        ep.S[r * ep.lds4 + e4] = o;
    }
    return yb;
}

template <int LPR>
__device__ __forceinline__ int wave_max_over_subgroups(int n) {
#pragma unroll
    for (int m = MI_WAVE / 2; m >= LPR; m >>= 1) n = max(n, __shfl_xor(n, m, MI_WAVE));
    return n;
}

// The calling sub-group of LPR lanes accumulates entries [beg, beg + n) in list order; lane li holds columns [8 li, 8 li + 8).
// nmax = the longest n of the wavefront's sub-groups (the shuffles need wave-uniform trip counts): a sub-group past its own
// end adds 0 * 0, which changes no sum.
template <int LPR>
__device__ __forceinline__ void subgroup_accumulate(const int32_t* __restrict__ col, const float* __restrict__ val,
                                                    const uint4* __restrict__ X, int64_t ldx8, int d8,
                                                    int32_t beg, int n, int nmax, int li, float (&acc)[8]) {
    static_assert(LPR % kUnroll == 0, "a batch of LPR entries is consumed kUnroll at a time");
#pragma unroll
    for (int v = 0; v < 8; ++v) acc[v] = 0.f;
    for (int base = 0; base < nmax; base += LPR) {
        int32_t my_c = -1;
        float my_v = 0.f;
        if (base + li < n) {
            my_c = col[beg + base + li];
            my_v = val[beg + base + li];
        }
        const int m = min(LPR, nmax - base);
        for (int j = 0; j < m; j += kUnroll) {
            float w[kUnroll];
            uint4 x[kUnroll];
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                const int32_t c = __shfl(my_c, j + u, LPR);
                w[u] = __shfl(my_v, j + u, LPR);
                const bool ok = c >= 0 && li < d8;
                x[u] = ok ? X[(int64_t)(c >= 0 ? c : 0) * ldx8 + li] : make_uint4(0u, 0u, 0u, 0u);
                if (!ok) w[u] = 0.f;
            }
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                acc[0] = fmaf(w[u], bf16_lo(x[u].x), acc[0]);
                acc[1] = fmaf(w[u], bf16_hi(x[u].x), acc[1]);
                acc[2] = fmaf(w[u], bf16_lo(x[u].y), acc[2]);
                acc[3] = fmaf(w[u], bf16_hi(x[u].y), acc[3]);
                acc[4] = fmaf(w[u], bf16_lo(x[u].z), acc[4]);
                acc[5] = fmaf(w[u], bf16_hi(x[u].z), acc[5]);
                acc[6] = fmaf(w[u], bf16_lo(x[u].w), acc[6]);
                acc[7] = fmaf(w[u], bf16_hi(x[u].w), acc[7]);
            }
        }
    }
}

// One sub-group per output row; rows with more than `chunk` entries belong to the work items and the fix-up.
template <int LPR, bool LISTED>
__global__ __launch_bounds__(kBlock) void spmm_bf16_rows_kernel(int64_t n_out, int d8, const int32_t* __restrict__ rowptr,
                                                                const int32_t* __restrict__ col,
                                                                const float* __restrict__ val,
                                                                const uint4* __restrict__ X, int64_t ldx8, Out ep,
                                                                int32_t chunk, const int32_t* __restrict__ row_list,
                                                                const int32_t* __restrict__ n_list_dev) {
    constexpr int NB = MI_WAVE / LPR, SG = NB * kWavesPerBlock;
    const int lane = mi_lane();
    const int li = lane % LPR;
    const int sgi = (threadIdx.x / MI_WAVE) * NB + lane / LPR;
    int64_t n_valid = n_out;
    if (LISTED && n_list_dev) n_valid = min(n_out, (int64_t)*n_list_dev);
    const int64_t i = (int64_t)blockIdx.x * SG + sgi;   // output position
    int32_t beg = 0;
    int n = 0;
    bool mine = i < n_valid;
    if (mine) {
        const int64_t r = LISTED ? (int64_t)row_list[i] : i;
        beg = rowptr[r];
        n = rowptr[r + 1] - beg;
        mine = n <= chunk;
    }
    if (!mine) n = 0;
    const int nmax = wave_max_over_subgroups<LPR>(n);
    float acc[8];
    subgroup_accumulate<LPR>(col, val, X, ldx8, d8, beg, n, nmax, li, acc);
    if (!mine || li >= d8) return;
    const uint2 y0 = finish4(ep, i, 2 * li, make_float4(acc[0], acc[1], acc[2], acc[3]));
    const uint2 y1 = finish4(ep, i, 2 * li + 1, make_float4(acc[4], acc[5], acc[6], acc[7]));
    if (ep.Y) *reinterpret_cast<uint4*>(ep.Y + i * ep.ldy + 8 * li) = make_uint4(y0.x, y0.y, y1.x, y1.y);
}

// Split rows: one sub-group per launch slot (row, begin, end, slot) -> partial[slot, :] in f32; slot < 0 = padding.  The slots
// are taken in the plan's launch order; on a banded plan workgroup w serves the queue of XCD w mod 8, as spmm_items_kernel does
// (`banded` is set only when a workgroup's SG slots divide a launch block).
template <int LPR>
__global__ __launch_bounds__(kBlock) void spmm_bf16_items_kernel(int64_t n_launch, int32_t n_items, int32_t banded, int d8,
                                                                 const int4* __restrict__ items,
                                                                 const int32_t* __restrict__ col,
                                                                 const float* __restrict__ val,
                                                                 const uint4* __restrict__ X, int64_t ldx8,
                                                                 float4* __restrict__ partial) {
    constexpr int NB = MI_WAVE / LPR, SG = NB * kWavesPerBlock;
    const int lane = mi_lane();
    const int li = lane % LPR;
    const int sgi = (threadIdx.x / MI_WAVE) * NB + lane / LPR;
    int64_t base = (int64_t)blockIdx.x * SG;
    if (banded) {
        constexpr int per = (kPlanGroup / SG) > 0 ? kPlanGroup / SG : 1;
        const int64_t x = blockIdx.x & 7, tq = blockIdx.x >> 3;
        base = ((tq / per) * 8 + x) * kPlanGroup + (tq % per) * SG;
    }
    const int64_t q = base + sgi;
    int4 it = make_int4(0, 0, 0, -1);
    if (q < n_launch) it = items[q];
    const int32_t slot = it.w;
    const bool live = slot >= 0 && slot < n_items;
    const int n = live ? it.z - it.y : 0;
    const int nmax = wave_max_over_subgroups<LPR>(n);
    float acc[8];
    subgroup_accumulate<LPR>(col, val, X, ldx8, d8, it.y, n, nmax, li, acc);
    if (!live || li >= d8) return;
    float4* p = partial + ((int64_t)slot * d8 + li) * 2;
    p[0] = make_float4(acc[0], acc[1], acc[2], acc[3]);
    p[1] = make_float4(acc[4], acc[5], acc[6], acc[7]);
}

// One workgroup per split row (per list position of a row-list launch): its sub-groups of LQ lanes (one float4 of the row per
// lane) stride over the row's partial rows in slot order, then combine across the wavefront's sub-groups and across the four
// wavefronts in a fixed order.  Wave 0 applies the epilogue.  The association depends on the row's slots alone, so the listed
// form gives the dense form's bits.
template <int LQ, bool LISTED>
__global__ __launch_bounds__(kBlock) void spmm_bf16_fixup_kernel(int32_t n_long, int d4, const int32_t* __restrict__ long_rows,
                                                                 const int32_t* __restrict__ item_ptr,
                                                                 const float4* __restrict__ partial, Out ep,
                                                                 const int32_t* __restrict__ row_list,
                                                                 const int32_t* __restrict__ n_list_dev,
                                                                 const int32_t* __restrict__ long_index) {
    constexpr int NB = MI_WAVE / LQ, NSG = NB * kWavesPerBlock;
    __shared__ float4 red[kWavesPerBlock][LQ];
    // every exit below depends on blockIdx only: the whole workgroup leaves together, before the barrier
    int32_t i = blockIdx.x;
    int64_t out_row;
    if (LISTED) {
        if (i >= n_long || (n_list_dev && i >= *n_list_dev)) return;
        out_row = i;
        i = long_index[row_list[i]];
        if (i < 0) return;   // a short row: the short-row kernel's
    } else {
        if (i >= n_long) return;
        out_row = long_rows[i];
    }
    const int32_t sb = item_ptr[i], se = item_ptr[i + 1];
    const int lane = mi_lane(), wave = threadIdx.x / MI_WAVE;
    const int li = lane % LQ, sg = wave * NB + lane / LQ;
    float4 acc = mi_f4_zero();
    for (int32_t s = sb + sg; s < se; s += NSG * kFixupUnroll) {
        float4 x[kFixupUnroll];
#pragma unroll
        for (int u = 0; u < kFixupUnroll; ++u) {
            const int32_t ss = s + u * NSG;
            x[u] = (ss < se && li < d4) ? partial[(int64_t)ss * d4 + li] : mi_f4_zero();
        }
#pragma unroll
        for (int u = 0; u < kFixupUnroll; ++u) acc = mi_f4_add(acc, x[u]);
    }
#pragma unroll
    for (int m = MI_WAVE / 2; m >= LQ; m >>= 1) acc = mi_f4_add(acc, mi_f4_shfl_xor(acc, m));
    if (lane < LQ) red[wave][lane] = acc;
    __syncthreads();
    if (wave != 0 || lane >= LQ || lane >= d4) return;
    float4 tot = red[0][lane];
#pragma unroll
    for (int w = 1; w < kWavesPerBlock; ++w) tot = mi_f4_add(tot, red[w][lane]);
    const uint2 yb = finish4(ep, out_row, lane, tot);
    if (ep.Y) *reinterpret_cast<uint2*>(ep.Y + out_row * ep.ldy + 4 * lane) = yb;
}

template <int LPR>
int launch_bf16(int64_t n_rows, int d, const int32_t* rowptr, const int32_t* col, const float* val, const uint4* X,
                int64_t ldx8, const Out& ep, const mi_spmm_plan* plan, float4* partial, const int32_t* row_list,
                const int32_t* n_list_dev, int64_t n_list, int32_t parts, hipStream_t s) {
    constexpr int SG = (MI_WAVE / LPR) * kWavesPerBlock;
    constexpr int LQ = 2 * LPR;   // float4 per partial row, rounded like the sub-group: 8 .. 64 lanes
    const int d8 = d / 8, d4 = d / 4;
    const bool listed = row_list != nullptr;
    const int32_t chunk = plan ? plan->chunk : INT32_MAX;
    const bool split = (parts & MI_SPMM_SPLIT_ROWS) && plan && plan->n_items > 0;
    if (split) {
        const int64_t n_launch = plan->n_launch;
        const int32_t banded = (plan->band > 0 && SG <= kPlanGroup) ? 1 : 0;
        hipLaunchKernelGGL((spmm_bf16_items_kernel<LPR>), dim3((unsigned)mi_ceil_div(n_launch, (int64_t)SG)), dim3(kBlock), 0, s,
                           n_launch, plan->n_items, banded, d8, reinterpret_cast<const int4*>(plan->items), col, val, X, ldx8,
                           partial);
    }
    const int64_t n_out = listed ? n_list : n_rows;
    if ((parts & MI_SPMM_SHORT_ROWS) && n_out > 0) {
        const dim3 g((unsigned)mi_ceil_div(n_out, (int64_t)SG));
        if (listed)
            hipLaunchKernelGGL((spmm_bf16_rows_kernel<LPR, true>), g, dim3(kBlock), 0, s, n_out, d8, rowptr, col, val, X, ldx8, ep,
                               chunk, row_list, n_list_dev);
        else
            hipLaunchKernelGGL((spmm_bf16_rows_kernel<LPR, false>), g, dim3(kBlock), 0, s, n_out, d8, rowptr, col, val, X, ldx8, ep,
                               chunk, row_list, n_list_dev);
    }
    if (split && plan->n_long_rows > 0) {
        const int64_t nf = listed ? n_list : (int64_t)plan->n_long_rows;
        if (listed)
            hipLaunchKernelGGL((spmm_bf16_fixup_kernel<LQ, true>), dim3((unsigned)nf), dim3(kBlock), 0, s, (int32_t)nf, d4,
                               plan->long_rows, plan->item_ptr, partial, ep, row_list, n_list_dev, plan->long_index);
        else
            hipLaunchKernelGGL((spmm_bf16_fixup_kernel<LQ, false>), dim3((unsigned)nf), dim3(kBlock), 0, s, (int32_t)nf, d4,
                               plan->long_rows, plan->item_ptr, partial, ep, row_list, n_list_dev, plan->long_index);
    }
    return mi_launch_status();
}

// Eight elements per thread: two 16-byte loads, one 16-byte store.
__global__ __launch_bounds__(kBlock) void rows_f32_to_bf16_kernel(int64_t n8, int d8, const float4* __restrict__ src, int64_t ld_src4,
                                                                  uint4* __restrict__ dst, int64_t ld_dst8) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n8) return;
    const int64_t r = i / d8;
    const int e = (int)(i % d8);
    const float4 a = src[r * ld_src4 + 2 * e], b = src[r * ld_src4 + 2 * e + 1];
    dst[r * ld_dst8 + e] = make_uint4(pack2(a.x, a.y), pack2(a.z, a.w), pack2(b.x, b.y), pack2(b.z, b.w));
}

__global__ __launch_bounds__(kBlock) void gather_rows_bf16_kernel(int64_t n_max, const int32_t* __restrict__ n_dev, int d8,
                                                                  const int32_t* __restrict__ rows, const uint4* __restrict__ src,
                                                                  int64_t ld_src8, float4* __restrict__ dst, int64_t ld_dst4,
                                                                  int32_t accumulate) {
    const int64_t n = n_dev ? min(n_max, (int64_t)*n_dev) : n_max;
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t i = t / d8;
    if (i >= n) return;
    const int e = (int)(t % d8);
    const uint4 x = src[(int64_t)rows[i] * ld_src8 + e];
    float4* out = dst + i * ld_dst4 + 2 * e;
    float4 a = make_float4(bf16_lo(x.x), bf16_hi(x.x), bf16_lo(x.y), bf16_hi(x.y));
    float4 b = make_float4(bf16_lo(x.z), bf16_hi(x.z), bf16_lo(x.w), bf16_hi(x.w));
    if (accumulate) {
        a = mi_f4_add(out[0], a);
        b = mi_f4_add(out[1], b);
    }
    out[0] = a;
    out[1] = b;
}

}  // namespace

extern "C" {

int mi_rows_f32_to_bf16(int64_t n_rows, int64_t d, const float* src, int64_t ld_src, uint16_t* dst, int64_t ld_dst,
                        mi_stream_t stream) {
    MI_CHECK_ARG(n_rows >= 0 && d > 0 && d % 8 == 0);
    if (n_rows == 0) return 0;
    MI_CHECK_ARG(src && dst && mi_aligned16(src) && mi_aligned16(dst));
    MI_CHECK_ARG(ld_src % 4 == 0 && ld_src >= d && ld_dst % 8 == 0 && ld_dst >= d);
    MI_CHECK_ARG((const void*)src != (const void*)dst);
    if (d / 8 > INT32_MAX) return MI_ERR_TOO_LARGE;
    const int64_t n8 = n_rows * (d / 8);
    if (mi_ceil_div(n8, (int64_t)kBlock) >= INT32_MAX) return MI_ERR_TOO_LARGE;
    hipLaunchKernelGGL(rows_f32_to_bf16_kernel, dim3((unsigned)mi_ceil_div(n8, (int64_t)kBlock)), dim3(kBlock), 0, (hipStream_t)stream,
                       n8, (int)(d / 8), reinterpret_cast<const float4*>(src), ld_src / 4, reinterpret_cast<uint4*>(dst), ld_dst / 8);
    return mi_launch_status();
}

int mi_gather_rows_bf16_f32(int64_t n_max, const int32_t* n_dev, int64_t d, const int32_t* rows, const uint16_t* src,
                            int64_t ld_src, float* dst, int64_t ld_dst, int32_t accumulate, mi_stream_t stream) {
    MI_CHECK_ARG(n_max >= 0 && d > 0 && d % 8 == 0);
    if (n_max == 0) return 0;
    MI_CHECK_ARG(rows && src && dst && mi_aligned16(src) && mi_aligned16(dst));
    MI_CHECK_ARG(ld_src % 8 == 0 && ld_src >= d && ld_dst % 4 == 0 && ld_dst >= d);
    if (d / 8 > INT32_MAX) return MI_ERR_TOO_LARGE;
    const int64_t n8 = n_max * (d / 8);
    if (mi_ceil_div(n8, (int64_t)kBlock) >= INT32_MAX) return MI_ERR_TOO_LARGE;
    hipLaunchKernelGGL(gather_rows_bf16_kernel, dim3((unsigned)mi_ceil_div(n8, (int64_t)kBlock)), dim3(kBlock), 0, (hipStream_t)stream,
                       n_max, n_dev, (int)(d / 8), rows, reinterpret_cast<const uint4*>(src), ld_src / 8,
                       reinterpret_cast<float4*>(dst), ld_dst / 4, accumulate);
    return mi_launch_status();
}

int mi_spmm_csr_bf16(int64_t n_rows, int64_t d, const int32_t* rowptr, const int32_t* col, const float* val,
                     const uint16_t* X, int64_t ldx, uint16_t* Y, int64_t ldy, const float* addend, int64_t lda,
                     float* S, int64_t lds, float scale, const mi_spmm_plan* plan, const int32_t* row_list,
                     const int32_t* n_list_dev, int64_t n_list, int32_t parts, void* ws, size_t ws_bytes, mi_stream_t stream) {
    MI_CHECK_ARG(n_rows >= 0 && d > 0 && d % 8 == 0 && rowptr);
    if (d > 256) return MI_ERR_UNSUPPORTED;
    if (n_rows == 0) return 0;
    if (n_rows >= INT32_MAX) return MI_ERR_TOO_LARGE;
    MI_CHECK_ARG(X && col && val && (Y || S));
    MI_CHECK_ARG(ldx % 8 == 0 && ldx >= d && mi_aligned16(X));
    MI_CHECK_ARG(!Y || (ldy % 8 == 0 && ldy >= d && mi_aligned16(Y) && Y != X));
    MI_CHECK_ARG(!S || (lds % 4 == 0 && lds >= d && mi_aligned16(S) && (const void*)S != (const void*)X));
    MI_CHECK_ARG(!addend || (lda % 4 == 0 && lda >= d && mi_aligned16(addend)));
    MI_CHECK_ARG((parts & ~(MI_SPMM_SHORT_ROWS | MI_SPMM_SPLIT_ROWS)) == 0);
    if (parts == 0) parts = MI_SPMM_SHORT_ROWS | MI_SPMM_SPLIT_ROWS;
    MI_CHECK_ARG(row_list || (!n_list_dev && n_list == 0));
    if (row_list) {
        MI_CHECK_ARG(n_list >= 0 && n_list < INT32_MAX);
        if (n_list == 0) return 0;
        MI_CHECK_ARG(!plan || plan->n_long_rows <= 0 || plan->long_index);
    }
    float4* partial = nullptr;
    if (plan) {
        MI_CHECK_ARG(plan->chunk > 0 && plan->n_items >= 0 && plan->n_long_rows >= 0);
        if (plan->n_items > 0) {
            MI_CHECK_ARG(plan->items && plan->item_ptr && plan->long_rows && plan->n_long_rows > 0);
            MI_CHECK_ARG(plan->n_launch >= plan->n_items && mi_aligned16(plan->items));
            MI_CHECK_ARG(plan->band == 0 || plan->n_launch % (8 * kPlanGroup) == 0);
            if (!ws || ws_bytes < mi_spmm_workspace_bytes(plan, d)) return MI_ERR_WORKSPACE;
            MI_CHECK_ARG(mi_aligned16(ws));
            partial = reinterpret_cast<float4*>(ws);
        }
    }
    Out ep;
    ep.Y = Y;                                            ep.ldy = ldy;
    ep.addend = reinterpret_cast<const float4*>(addend); ep.lda4 = lda / 4;
    ep.S = reinterpret_cast<float4*>(S);                 ep.lds4 = lds / 4;
    ep.scale = scale;
    const uint4* X8 = reinterpret_cast<const uint4*>(X);
    hipStream_t s = (hipStream_t)stream;
    const int di = (int)d;
#define MI_BF16_GO(LPR) \
    return launch_bf16<LPR>(n_rows, di, rowptr, col, val, X8, ldx / 8, ep, plan, partial, row_list, n_list_dev, n_list, parts, s)
    if (d <= 32) MI_BF16_GO(4);
    if (d <= 64) MI_BF16_GO(8);
    if (d <= 128) MI_BF16_GO(16);
    MI_BF16_GO(32);
#undef MI_BF16_GO
}

}  // extern "C"
