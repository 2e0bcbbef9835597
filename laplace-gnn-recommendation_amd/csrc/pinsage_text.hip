// N5: bag-of-words text columns of PinSAGE's item feature projector (mi_pinsage_text_f32 / _bwd_f32 / _clear_f32;
// include/laplace_hip.h, additive to ABI 14).
//
//   bag_c[r] = ((E_c[tok[p0]] + E_c[tok[p0 + 1]]) + ...) / (float)len,   p0 = ptr_c[i], len = ptr_c[i + 1] - p0,   i = ids ? ids[r] : r
//   out[r]   = (out[r] +) bag_0[r] + bag_1[r] + ...
//
// (restates the reference's BagOfWords, pinsage/layers.py:49-87: the mean of an embedding row per token; an empty bag is
// zero here).  The forward is a variable-length gather-mean, one lane per float4 of an output row, 8 token rows in flight.
//
// Backward: g_tables[c][v] = sum over the references (r, position) with token v of g[r] / (float)len(i_r).  One token of a
// small vocabulary is referenced by thousands of positions of a block, so this is the segmented sum of pinsage_proj.hip with
// two differences: the references of a call are counted on the device (lengths -> exclusive scan -> one thread per reference
// finds its (column, row) by bisection; slots past the count up to the caller's bound get a key that sorts last and are never
// read), and every reference carries the scale 1 / len of its row, applied as a division before the sum (DivByLen).  The
// references are written in (column, r) order, then the position in the bag; the sort, the chunks of 64 and the combine
// are segsum.hpp's.
#include "segsum.hpp"
#include "lazy_adam.hpp"

namespace {

constexpr int kBlock = 256;
constexpr int kTok = 8;          // token rows a lane keeps in flight (forward)
constexpr int kT = MI_PROJECTOR_MAX_TEXT;

inline unsigned grid_for(int64_t n) { return (unsigned)mi_ceil_div(n > 0 ? n : 1, kBlock); }

struct TextCsr {   // by value in the kernel arguments
    segsum::Ptrs<const int64_t, kT> ptr;
    segsum::Ptrs<const int32_t, kT> tok;
};
using TextTables = segsum::Ptrs<const float4, kT>;
using TextGradTables = segsum::Ptrs<float4, kT>;

__device__ __forceinline__ float4 f4_div(const float4& a, float d) {
    return make_float4(__fdiv_rn(a.x, d), __fdiv_rn(a.y, d), __fdiv_rn(a.z, d), __fdiv_rn(a.w, d));
}

// ---- forward ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void text_gather_kernel(int64_t n, int w4, int n_text, const int64_t* __restrict__ ids,
                                                             TextCsr csr, TextTables tabs, float4* __restrict__ out,
                                                             int64_t ldo4, int accumulate) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n * w4) return;
    const int64_t r = i / w4;
    const int e = (int)(i - r * w4);
    const int64_t item = ids ? ids[r] : r;
    float4 acc = mi_f4_zero();
    bool first = true;
    if (accumulate) {
        acc = out[r * ldo4 + e];
        first = false;
    }
#pragma unroll
    for (int c = 0; c < kT; ++c) {
        if (c < n_text) {
            const int64_t p0 = csr.ptr.t[c][item], p1 = csr.ptr.t[c][item + 1];
            const int32_t* __restrict__ tok = csr.tok.t[c];
            const float4* __restrict__ tab = tabs.t[c];
            float4 bag = mi_f4_zero();
            for (int64_t q0 = p0; q0 < p1; q0 += kTok) {
                int32_t tk[kTok];
                float4 rows[kTok];
#pragma unroll
                for (int u = 0; u < kTok; ++u) tk[u] = tok[min(q0 + u, p1 - 1)];
#pragma unroll
                for (int u = 0; u < kTok; ++u) rows[u] = tab[(int64_t)tk[u] * w4 + e];
#pragma unroll
                for (int u = 0; u < kTok; ++u) {
                    if (q0 + u < p1) bag = (q0 + u == p0) ? rows[u] : mi_f4_add(bag, rows[u]);
                }
            }
            if (p1 > p0) bag = f4_div(bag, (float)(p1 - p0));
            acc = first ? bag : mi_f4_add(acc, bag);
            first = false;
        }
    }
    out[r * ldo4 + e] = acc;
}

// ---- backward: references ------------------------------------------------------------------------------------------------
// lens[c * n + r] = the length of row r's bag in column c
__global__ __launch_bounds__(kBlock) void text_lens_kernel(int64_t n, int64_t n_pairs, const int64_t* __restrict__ ids, TextCsr csr,
                                                           int64_t* __restrict__ lens) {
    const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (q >= n_pairs) return;
    const int c = (int)(q / n);
    const int64_t r = q - (int64_t)c * n;
    const int64_t item = ids ? ids[r] : r;
    const int64_t* ptr = csr.ptr.at(c);
    lens[q] = ptr[item + 1] - ptr[item];
}

// One thread per reference slot j < n_ref_max.  Reference j of the call is (pair q, position j - off[q]) for the last pair q
// with off[q] <= j: pairs in (column, r) order, so that the stable sort keeps ascending (r, position) within a token.
__global__ __launch_bounds__(kBlock) void text_refs_kernel(int64_t n, int64_t n_pairs, int64_t n_ref_max, const int64_t* __restrict__ ids,
                                                           TextCsr csr, const int64_t* __restrict__ lens,
                                                           const int64_t* __restrict__ off, unsigned shift, uint64_t pad_key,
                                                           uint64_t* __restrict__ keys, uint32_t* __restrict__ refs,
                                                           int64_t* __restrict__ count) {
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t total = off[n_pairs - 1] + lens[n_pairs - 1];
    if (j == 0) *count = total;
    if (j >= n_ref_max) return;
    if (j >= total) {
        keys[j] = pad_key;
        refs[j] = 0u;
        return;
    }
    int64_t lo = 0, hi = n_pairs;   // the first pair with off > j
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (off[mid] <= j) lo = mid + 1;
        else hi = mid;
    }
    const int64_t q = lo - 1;
    const int c = (int)(q / n);
    const int64_t r = q - (int64_t)c * n;
    const int64_t item = ids ? ids[r] : r;
    const int64_t p = csr.ptr.at(c)[item] + (j - off[q]);
    keys[j] = ((uint64_t)c << shift) | (uint64_t)(uint32_t)csr.tok.at(c)[p];
    refs[j] = (uint32_t)r;
}

// The term of a reference (segsum::chunk_kernel): the length of its row's bag, loaded beside the row of g; the row is divided by
// it before the add.
struct DivByLen {
    const int64_t* lens;   // [column * n + r]
    int64_t n;
    using Loaded = float;
    __device__ __forceinline__ float load(uint64_t key, uint32_t r, unsigned shift) const {
        return (float)lens[(int64_t)(key >> shift) * n + r];
    }
    __device__ __forceinline__ float4 apply(const float4& row, float len) const { return f4_div(row, len); }
};

// The rows the backward wrote, back to zero: one lane group per (column, r), every token of its bag (every writer stores the
// same zeros).
__global__ __launch_bounds__(kBlock) void text_clear_kernel(int64_t n, int64_t n_pairs, int w4, int lpr, const int64_t* __restrict__ ids,
                                                            TextCsr csr, TextGradTables gt) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t q = t / lpr;
    const int e = (int)(t - q * lpr);
    if (q >= n_pairs || e >= w4) return;
    const int c = (int)(q / n);
    const int64_t r = q - (int64_t)c * n;
    const int64_t item = ids ? ids[r] : r;
    const int64_t* ptr = csr.ptr.at(c);
    const int32_t* tok = csr.tok.at(c);
    float4* tab = gt.at(c);
    const int64_t p1 = ptr[item + 1];
    for (int64_t p = ptr[item]; p < p1; ++p) tab[(int64_t)tok[p] * w4 + e] = mi_f4_zero();
}

// ---- host ------------------------------------------------------------------------------------------------------------------
// Everything about the descriptor that does not depend on the call's buffers.  0, or the code to return.
int check_text(const mi_text_columns* pp, int64_t n, bool has_ids) {
    if (!pp) return MI_ERR_BAD_ARG;
    const mi_text_columns& p = *pp;
    if (p.width < 4 || p.width % 4 != 0 || p.width > 512) return MI_ERR_UNSUPPORTED;
    if (p.n_text > kT) return MI_ERR_UNSUPPORTED;
    if (p.n_text < 1 || p.n_items < 1 || n < 0) return MI_ERR_BAD_ARG;
    if (!has_ids && n > p.n_items) return MI_ERR_BAD_ARG;
    for (int c = 0; c < p.n_text; ++c) {
        if (!p.ptr[c] || !p.tok[c] || !p.tables[c] || p.vocab[c] < 1) return MI_ERR_BAD_ARG;
        if ((reinterpret_cast<uintptr_t>(p.ptr[c]) & 7u) || (reinterpret_cast<uintptr_t>(p.tok[c]) & 3u) || !mi_aligned16(p.tables[c]))
            return MI_ERR_BAD_ARG;
        if (p.vocab[c] > (int64_t)INT32_MAX) return MI_ERR_TOO_LARGE;
    }
    if (p.n_items >= ((int64_t)1 << 40) || n * (int64_t)kT >= INT32_MAX) return MI_ERR_TOO_LARGE;
    return 0;
}

int check_text_grads(const mi_text_columns& p, float* const g_tables[]) {
    if (!g_tables) return MI_ERR_BAD_ARG;
    for (int c = 0; c < p.n_text; ++c)
        if (!g_tables[c] || !mi_aligned16(g_tables[c])) return MI_ERR_BAD_ARG;
    return 0;
}

TextCsr csr_of(const mi_text_columns& p) {
    TextCsr z;
    for (int c = 0; c < kT; ++c) {
        z.ptr.t[c] = c < p.n_text ? p.ptr[c] : nullptr;
        z.tok.t[c] = c < p.n_text ? p.tok[c] : nullptr;
    }
    return z;
}

TextGradTables grad_tables(const mi_text_columns& p, float* const g_tables[]) {
    TextGradTables gt;
    for (int c = 0; c < kT; ++c) gt.t[c] = c < p.n_text ? reinterpret_cast<float4*>(g_tables[c]) : nullptr;
    return gt;
}

// rocprim's temporary storage, shared by the scan (first) and the sort: a bound that grows with both counts
size_t tmp_cap(int64_t n_pairs, int64_t n_ref) {
    return ((size_t)3 << 20) + mi_align_up((size_t)n_ref * 4, 256) + mi_align_up((size_t)n_pairs, 256);
}

size_t bwd_ws_bytes(const mi_text_columns& p, int64_t n, int64_t n_ref_max) {
    const int64_t n_pairs = n * p.n_text;
    const size_t np = (size_t)std::max<int64_t>(n_pairs, 1);
    return 256 + 2 * mi_align_up(np * sizeof(int64_t), 256) +          // the count; lens, off
           segsum::workspace_bytes(n_ref_max, p.width, tmp_cap(n_pairs, n_ref_max));
}

// mi_pinsage_text_bwd_f32 (m_tables == nullptr) and mi_pinsage_text_bwd_lazy_f32: one body, the same bits in the gradients.  A
// column with a moment pair gets the lazy update over the heads of the sorted keys after the combine; the padding slots past
// the device-side count are behind head_kernel's own bound and never head a run.
static int text_bwd(const mi_text_columns* pp, float* const g_tables[], float* const m_tables[], float* const v_tables[],
                    const mi_lazy_adam* lazy, int64_t n, const int64_t* ids, const float* g, int64_t ldg, int64_t n_ref_max, void* ws,
                    size_t ws_bytes, mi_stream_t stream) {
    int bad = check_text(pp, n, ids != nullptr);
    if (bad) return bad;
    const mi_text_columns& p = *pp;
    bad = check_text_grads(p, g_tables);
    if (bad) return bad;
    MiLazyRowOp<segsum::Ptrs<float4, kT>> op = {};
    bool any_lazy = false;
    if (m_tables || v_tables) {
        if (!m_tables || !v_tables) return MI_ERR_BAD_ARG;
        for (int c = 0; c < kT; ++c) op.p.t[c] = op.m.t[c] = op.v.t[c] = nullptr;
        for (int c = 0; c < p.n_text; ++c) {
            float *m = m_tables[c], *v = v_tables[c];
            if ((m == nullptr) != (v == nullptr)) return MI_ERR_BAD_ARG;
            if (!m) continue;
            if (!mi_aligned16(m) || !mi_aligned16(v)) return MI_ERR_BAD_ARG;
            op.p.t[c] = reinterpret_cast<float4*>(const_cast<float*>(p.tables[c]));   // a lazy column's table is written
            op.m.t[c] = reinterpret_cast<float4*>(m);
            op.v.t[c] = reinterpret_cast<float4*>(v);
            any_lazy = true;
        }
        if (any_lazy) {
            bad = mi_lazy_check(lazy);
            if (bad) return bad;
            op.c = mi_lazy_consts(*lazy);
        }
    }
    MI_CHECK_ARG(n_ref_max >= 0);
    if (n_ref_max >= INT32_MAX) return MI_ERR_TOO_LARGE;
    MI_CHECK_ARG(n == 0 || (g && mi_aligned16(g) && ldg >= p.width && ldg % 4 == 0));
    if (!ws || !mi_aligned16(ws) || ws_bytes < bwd_ws_bytes(p, n, n_ref_max)) return MI_ERR_WORKSPACE;
    const int64_t n_pairs = n * p.n_text, n_ref = n_ref_max;
    hipStream_t s = (hipStream_t)stream;
    MiArena arena(ws, ws_bytes);
    int64_t* count = arena.take<int64_t>(1);
    int64_t* lens = arena.take<int64_t>(std::max<int64_t>(n_pairs, 1));
    int64_t* off = arena.take<int64_t>(std::max<int64_t>(n_pairs, 1));
    const segsum::Buffers sb = segsum::take(arena, n_ref, p.width, tmp_cap(n_pairs, n_ref));
    if (!count || !lens || !off || !sb.ok()) return MI_ERR_WORKSPACE;
    if (n_pairs == 0 || n_ref == 0) {   // no row, or a bound that says no reference: nothing to write
        MI_HIP(hipMemsetAsync(count, 0, sizeof(int64_t), s));
        return 0;
    }
    // the key: column above `shift` bits of token; column n_text is the padding of the slots past the actual count
    int64_t widest = 1;
    for (int c = 0; c < p.n_text; ++c) widest = std::max(widest, p.vocab[c]);
    const unsigned shift = mi_bits_for(widest), bits = shift + mi_bits_for(kT + 1);
    const uint64_t pad_key = (uint64_t)p.n_text << shift;
    size_t need_scan = 0;   // the size query enqueues nothing
    MI_HIP(rocprim::exclusive_scan(nullptr, need_scan, lens, off, (int64_t)0, (size_t)n_pairs, rocprim::plus<int64_t>(), s));
    auto refs = [&]() -> int {   // lengths -> offsets (the scan uses tmp before the sort does) -> references and their count
        const TextCsr csr = csr_of(p);
        hipLaunchKernelGGL(text_lens_kernel, dim3(grid_for(n_pairs)), dim3(kBlock), 0, s, n, n_pairs, ids, csr, lens);
        MI_HIP(rocprim::exclusive_scan(sb.tmp, need_scan, lens, off, (int64_t)0, (size_t)n_pairs, rocprim::plus<int64_t>(), s));
        hipLaunchKernelGGL(text_refs_kernel, dim3(grid_for(n_ref)), dim3(kBlock), 0, s, n, n_pairs, n_ref, ids, csr, lens, off, shift,
                           pad_key, sb.k0, sb.r0, count);
        return 0;
    };
    const uint64_t* sorted = nullptr;
    const int rc = segsum::run<true>(sb, n_ref, count, shift, bits, need_scan, refs, g, ldg, p.width, DivByLen{lens, n},
                                     grad_tables(p, g_tables), s, &sorted);
    if (rc || !any_lazy) return rc;
    return segsum::run_heads<true>(sorted, n_ref, count, shift, p.width, grad_tables(p, g_tables), op, s);
}

}  // namespace

extern "C" {

int64_t mi_pinsage_text_sizeof(int32_t which) { return which == 0 ? (int64_t)sizeof(mi_text_columns) : -1; }

int mi_pinsage_text_f32(const mi_text_columns* pp, int64_t n, const int64_t* ids, float* out, int64_t ldo, int32_t accumulate,
                        mi_stream_t stream) {
    const int bad = check_text(pp, n, ids != nullptr);
    if (bad) return bad;
    const mi_text_columns& p = *pp;
    MI_CHECK_ARG(accumulate == 0 || accumulate == 1);
    if (n == 0) return 0;
    MI_CHECK_ARG(out && mi_aligned16(out) && ldo >= p.width && ldo % 4 == 0);
    const int w4 = p.width / 4;
    if (n * (int64_t)w4 >= ((int64_t)INT32_MAX) * kBlock) return MI_ERR_TOO_LARGE;
    TextTables tabs;
    for (int c = 0; c < kT; ++c) tabs.t[c] = c < p.n_text ? reinterpret_cast<const float4*>(p.tables[c]) : nullptr;
    hipLaunchKernelGGL(text_gather_kernel, dim3(grid_for(n * w4)), dim3(kBlock), 0, (hipStream_t)stream, n, w4, (int)p.n_text, ids,
                       csr_of(p), tabs, reinterpret_cast<float4*>(out), ldo / 4, (int)accumulate);
    return mi_launch_status();
}

size_t mi_pinsage_text_bwd_workspace_bytes(const mi_text_columns* p, int64_t n, int64_t n_ref_max) {
    if (check_text(p, n, true) != 0 || n_ref_max < 0 || n_ref_max >= INT32_MAX) return 0;
    return bwd_ws_bytes(*p, n, n_ref_max);
}

int mi_pinsage_text_bwd_f32(const mi_text_columns* pp, float* const g_tables[], int64_t n, const int64_t* ids, const float* g,
                            int64_t ldg, int64_t n_ref_max, void* ws, size_t ws_bytes, mi_stream_t stream) {
    return text_bwd(pp, g_tables, nullptr, nullptr, nullptr, n, ids, g, ldg, n_ref_max, ws, ws_bytes, stream);
}

int mi_pinsage_text_bwd_lazy_f32(const mi_text_columns* pp, float* const g_tables[], float* const m_tables[], float* const v_tables[],
                                 const mi_lazy_adam* lazy, int64_t n, const int64_t* ids, const float* g, int64_t ldg,
                                 int64_t n_ref_max, void* ws, size_t ws_bytes, mi_stream_t stream) {
    return text_bwd(pp, g_tables, m_tables, v_tables, lazy, n, ids, g, ldg, n_ref_max, ws, ws_bytes, stream);
}

int mi_pinsage_text_clear_f32(const mi_text_columns* pp, float* const g_tables[], int64_t n, const int64_t* ids, mi_stream_t stream) {
    int bad = check_text(pp, n, ids != nullptr);
    if (bad) return bad;
    const mi_text_columns& p = *pp;
    bad = check_text_grads(p, g_tables);
    if (bad) return bad;
    const int64_t n_pairs = n * p.n_text;
    if (n_pairs == 0) return 0;
    const int w4 = p.width / 4, lpr = segsum::lanes_per_row(w4);
    hipLaunchKernelGGL(text_clear_kernel, dim3(grid_for(n_pairs * lpr)), dim3(kBlock), 0, (hipStream_t)stream, n, n_pairs, w4, lpr, ids,
                       csr_of(p), grad_tables(p, g_tables));
    return mi_launch_status();
}

}  // extern "C"
