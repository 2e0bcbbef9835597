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
// read), and every reference carries the scale 1 / len of its row, applied as a division before the sum.  Then as there: a
// stable radix sort of the (column, token) keys with the row as payload, chunks of 64 references, one lane group per chunk;
// a run inside a chunk is summed in order and stored by that group alone, a run that crosses chunk borders leaves one
// partial per chunk and the group of the chunk where it starts adds them in chunk order.  One writer per row, no float atomics.
#include "common.hpp"
#include <rocprim/rocprim.hpp>
#include <algorithm>

namespace {

constexpr int kBlock = 256;
constexpr int kChunk = 64;       // references per chunk
constexpr int kInFlight = 16;    // rows of g a lane group keeps in flight (backward)
constexpr int kTok = 8;          // token rows a lane keeps in flight (forward)
constexpr int kT = MI_PROJECTOR_MAX_TEXT;

inline unsigned grid_for(int64_t n) { return (unsigned)mi_ceil_div(n > 0 ? n : 1, kBlock); }

struct TextCsr {   // by value in the kernel arguments
    const int64_t* ptr[kT];
    const int32_t* tok[kT];
};
struct TextTables {
    const float4* t[kT];
};
struct TextGradTables {
    float4* t[kT];
};

// selects, no dynamically indexed copy of a kernel argument
template <typename T>
__device__ __forceinline__ T* pick(T* const (&a)[kT], int c) {
    T* p = a[0];
#pragma unroll
    for (int s = 1; s < kT; ++s) p = (s == c) ? a[s] : p;
    return p;
}

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
            const int64_t p0 = csr.ptr[c][item], p1 = csr.ptr[c][item + 1];
            const int32_t* __restrict__ tok = csr.tok[c];
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
    const int64_t* ptr = pick(csr.ptr, c);
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
    const int64_t p = pick(csr.ptr, c)[item] + (j - off[q]);
    keys[j] = ((uint64_t)c << shift) | (uint64_t)(uint32_t)pick(csr.tok, c)[p];
    refs[j] = (uint32_t)r;
}

// One group of `lpr` lanes (a power of two >= width / 4) per chunk of 64 sorted references.
__global__ __launch_bounds__(kBlock) void text_chunk_kernel(int64_t n, int64_t n_ref_max, const int64_t* __restrict__ count, int w4,
                                                            int lpr, unsigned shift, const uint64_t* __restrict__ keys,
                                                            const uint32_t* __restrict__ refs, const int64_t* __restrict__ lens,
                                                            const float4* __restrict__ g, int64_t ldg4, TextGradTables gt,
                                                            float4* __restrict__ part_head, float4* __restrict__ part_tail) {
    __shared__ float4* tab[kT];
    if (threadIdx.x < kT) tab[threadIdx.x] = pick(gt.t, (int)threadIdx.x);
    __syncthreads();
    const int64_t n_ref = min(*count, n_ref_max);
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t chunk = t / lpr;
    const int e = (int)(t - chunk * lpr);
    const int64_t j0 = chunk * kChunk;
    if (j0 >= n_ref || e >= w4) return;
    const int n_here = (int)min((int64_t)kChunk, n_ref - j0);
    const bool head_open = j0 > 0 && keys[j0 - 1] == keys[j0];
    const bool next_same = (j0 + n_here < n_ref) && keys[j0 + n_here] == keys[j0 + n_here - 1];
    const uint64_t mask = ((uint64_t)1 << shift) - 1;
    float4 acc = mi_f4_zero();
    int run_start = 0;
    // Two dependent loads per reference (its row index, then its row of g and its length): the indices and keys of step
    // s + 1 are fetched while the rows of step s are in flight.
    uint64_t kn[kInFlight + 1];
    uint32_t rn[kInFlight];
#pragma unroll
    for (int u = 0; u <= kInFlight; ++u) kn[u] = keys[j0 + min(u, n_here - 1)];
#pragma unroll
    for (int u = 0; u < kInFlight; ++u) rn[u] = refs[j0 + min(u, n_here - 1)];
    for (int q0 = 0; q0 < n_here; q0 += kInFlight) {
        uint64_t kq[kInFlight + 1];
        float4 rows[kInFlight];
        float len[kInFlight];
#pragma unroll
        for (int u = 0; u <= kInFlight; ++u) kq[u] = kn[u];
#pragma unroll
        for (int u = 0; u < kInFlight; ++u) {
            rows[u] = g[(int64_t)rn[u] * ldg4 + e];
            len[u] = (float)lens[(int64_t)(kq[u] >> shift) * n + rn[u]];
        }
        const int q1 = q0 + kInFlight;
        if (q1 < n_here) {
#pragma unroll
            for (int u = 0; u <= kInFlight; ++u) kn[u] = keys[j0 + min(q1 + u, n_here - 1)];
#pragma unroll
            for (int u = 0; u < kInFlight; ++u) rn[u] = refs[j0 + min(q1 + u, n_here - 1)];
        }
#pragma unroll
        for (int u = 0; u < kInFlight; ++u) {
            const int q = q0 + u;
            if (q >= n_here) break;
            acc = mi_f4_add(acc, f4_div(rows[u], len[u]));
            const bool last_of_run = (q + 1 == n_here) || kq[u + 1] != kq[u];
            if (!last_of_run) continue;
            const bool from_prev = run_start == 0 && head_open;
            const bool into_next = (q + 1 == n_here) && next_same;
            float4* dst;
            if (from_prev) dst = part_head + chunk * w4;          // finished by the chunk where the run starts
            else if (into_next) dst = part_tail + chunk * w4;     // this chunk starts the run; text_combine_kernel finishes it
            else dst = tab[kq[u] >> shift] + (int64_t)(kq[u] & mask) * w4;   // the row's only writer
            dst[e] = acc;
            acc = mi_f4_zero();
            run_start = q + 1;
        }
    }
}

// One lane group per chunk whose trailing run starts in it and runs on: tail partial + the head partials of the following
// chunks, in chunk order.
__global__ __launch_bounds__(kBlock) void text_combine_kernel(int64_t n_ref_max, const int64_t* __restrict__ count, int w4, int lpr,
                                                              unsigned shift, const uint64_t* __restrict__ keys, TextGradTables gt,
                                                              const float4* __restrict__ part_head,
                                                              const float4* __restrict__ part_tail) {
    const int64_t n_ref = min(*count, n_ref_max);
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t chunk = t / lpr;
    const int e = (int)(t - chunk * lpr);
    const int64_t j0 = chunk * kChunk;
    if (j0 >= n_ref || e >= w4) return;
    const int64_t j_last = min(j0 + kChunk, n_ref) - 1;
    if (j_last + 1 >= n_ref) return;                        // nothing after this chunk
    const uint64_t key = keys[j_last];
    if (keys[j_last + 1] != key) return;                    // the trailing run ends here
    if (keys[j0] == key && j0 > 0 && keys[j0 - 1] == key) return;   // the run started in an earlier chunk: not the owner
    float4 acc = part_tail[chunk * w4 + e];
    for (int64_t nb = chunk + 1; nb * kChunk < n_ref && keys[nb * kChunk] == key; ++nb) {
        acc = mi_f4_add(acc, part_head[nb * w4 + e]);
        if (keys[min((nb + 1) * kChunk, n_ref) - 1] != key) break;   // the run ends inside chunk nb
    }
    const uint64_t mask = ((uint64_t)1 << shift) - 1;
    pick(gt.t, (int)(key >> shift))[(int64_t)(key & mask) * w4 + e] = acc;
}

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
    const int64_t* ptr = pick(csr.ptr, c);
    const int32_t* tok = pick(csr.tok, c);
    float4* tab = pick(gt.t, c);
    const int64_t p1 = ptr[item + 1];
    for (int64_t p = ptr[item]; p < p1; ++p) tab[(int64_t)tok[p] * w4 + e] = mi_f4_zero();
}

// ---- host ------------------------------------------------------------------------------------------------------------------
inline unsigned bits_for(int64_t n) {   // bits that hold every value of [0, n)
    unsigned b = 1;
    while (b < 62 && ((int64_t)1 << b) < n) ++b;
    return b;
}

inline int lanes_per_row(int w4) {
    int l = 4;
    while (l < w4) l *= 2;
    return l;
}

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
        z.ptr[c] = c < p.n_text ? p.ptr[c] : nullptr;
        z.tok[c] = c < p.n_text ? p.tok[c] : nullptr;
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

struct BwdSizes {
    int64_t n_pairs, n_ref, n_chunks;
};
BwdSizes bwd_sizes(const mi_text_columns& p, int64_t n, int64_t n_ref_max) {
    BwdSizes z;
    z.n_pairs = n * p.n_text;
    z.n_ref = n_ref_max;
    z.n_chunks = mi_ceil_div(n_ref_max, kChunk);
    return z;
}
size_t bwd_ws_bytes(const mi_text_columns& p, int64_t n, int64_t n_ref_max) {
    const BwdSizes z = bwd_sizes(p, n, n_ref_max);
    const size_t np = (size_t)std::max<int64_t>(z.n_pairs, 1), nr = (size_t)std::max<int64_t>(z.n_ref, 1);
    const size_t nc = (size_t)std::max<int64_t>(z.n_chunks, 1);
    size_t total = 256;                                                     // the count
    total += 2 * mi_align_up(np * sizeof(int64_t), 256);                    // lens, off
    total += 2 * mi_align_up(nr * sizeof(uint64_t), 256) + 2 * mi_align_up(nr * sizeof(uint32_t), 256);
    total += mi_align_up(tmp_cap(z.n_pairs, z.n_ref), 256);
    total += 2 * mi_align_up(nc * p.width * sizeof(float), 256);
    return total;
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
    int bad = check_text(pp, n, ids != nullptr);
    if (bad) return bad;
    const mi_text_columns& p = *pp;
    bad = check_text_grads(p, g_tables);
    if (bad) return bad;
    MI_CHECK_ARG(n_ref_max >= 0);
    if (n_ref_max >= INT32_MAX) return MI_ERR_TOO_LARGE;
    MI_CHECK_ARG(n == 0 || (g && mi_aligned16(g) && ldg >= p.width && ldg % 4 == 0));
    if (!ws || !mi_aligned16(ws) || ws_bytes < bwd_ws_bytes(p, n, n_ref_max)) return MI_ERR_WORKSPACE;
    const BwdSizes z = bwd_sizes(p, n, n_ref_max);
    const int W = p.width, w4 = W / 4;
    hipStream_t s = (hipStream_t)stream;
    MiArena arena(ws, ws_bytes);
    int64_t* count = arena.take<int64_t>(1);
    int64_t* lens = arena.take<int64_t>(std::max<int64_t>(z.n_pairs, 1));
    int64_t* off = arena.take<int64_t>(std::max<int64_t>(z.n_pairs, 1));
    uint64_t* k0 = arena.take<uint64_t>(std::max<int64_t>(z.n_ref, 1));
    uint64_t* k1 = arena.take<uint64_t>(std::max<int64_t>(z.n_ref, 1));
    uint32_t* r0 = arena.take<uint32_t>(std::max<int64_t>(z.n_ref, 1));
    uint32_t* r1 = arena.take<uint32_t>(std::max<int64_t>(z.n_ref, 1));
    const size_t cap = tmp_cap(z.n_pairs, z.n_ref);
    char* tmp = arena.take<char>(cap);
    float* part_head = arena.take<float>((size_t)std::max<int64_t>(z.n_chunks, 1) * W);
    float* part_tail = arena.take<float>((size_t)std::max<int64_t>(z.n_chunks, 1) * W);
    if (!count || !lens || !off || !k0 || !k1 || !r0 || !r1 || !tmp || !part_head || !part_tail) return MI_ERR_WORKSPACE;
    if (z.n_pairs == 0 || z.n_ref == 0) {   // no row, or a bound that says no reference: nothing to write
        MI_HIP(hipMemsetAsync(count, 0, sizeof(int64_t), s));
        return 0;
    }
    // the key: column above `shift` bits of token; column n_text is the padding of the slots past the actual count
    int64_t widest = 1;
    for (int c = 0; c < p.n_text; ++c) widest = std::max(widest, p.vocab[c]);
    const unsigned shift = bits_for(widest), bits = shift + bits_for(kT + 1);
    const uint64_t pad_key = (uint64_t)p.n_text << shift;
    rocprim::double_buffer<uint64_t> keys(k0, k1);
    rocprim::double_buffer<uint32_t> refs(r0, r1);
    size_t need_scan = 0, need_sort = 0;   // the size queries enqueue nothing
    MI_HIP(rocprim::exclusive_scan(nullptr, need_scan, lens, off, (int64_t)0, (size_t)z.n_pairs, rocprim::plus<int64_t>(), s));
    MI_HIP(rocprim::radix_sort_pairs(nullptr, need_sort, keys, refs, (size_t)z.n_ref, 0u, bits, s));
    if (need_scan > cap || need_sort > cap) return MI_ERR_WORKSPACE;
    // ---- nothing has been enqueued up to here ----
    const TextCsr csr = csr_of(p);
    const TextGradTables gt = grad_tables(p, g_tables);
    const int lpr = lanes_per_row(w4);
    hipLaunchKernelGGL(text_lens_kernel, dim3(grid_for(z.n_pairs)), dim3(kBlock), 0, s, n, z.n_pairs, ids, csr, lens);
    MI_HIP(rocprim::exclusive_scan(tmp, need_scan, lens, off, (int64_t)0, (size_t)z.n_pairs, rocprim::plus<int64_t>(), s));
    hipLaunchKernelGGL(text_refs_kernel, dim3(grid_for(z.n_ref)), dim3(kBlock), 0, s, n, z.n_pairs, z.n_ref, ids, csr, lens, off, shift,
                       pad_key, k0, r0, count);
    MI_HIP(rocprim::radix_sort_pairs(tmp, need_sort, keys, refs, (size_t)z.n_ref, 0u, bits, s));
    const dim3 gc(grid_for(z.n_chunks * lpr));
    hipLaunchKernelGGL(text_chunk_kernel, gc, dim3(kBlock), 0, s, n, z.n_ref, count, w4, lpr, shift, keys.current(), refs.current(),
                       lens, reinterpret_cast<const float4*>(g), ldg / 4, gt, reinterpret_cast<float4*>(part_head),
                       reinterpret_cast<float4*>(part_tail));
    hipLaunchKernelGGL(text_combine_kernel, gc, dim3(kBlock), 0, s, z.n_ref, count, w4, lpr, shift, keys.current(), gt,
                       reinterpret_cast<const float4*>(part_head), reinterpret_cast<const float4*>(part_tail));
    return mi_launch_status();
}

int mi_pinsage_text_clear_f32(const mi_text_columns* pp, float* const g_tables[], int64_t n, const int64_t* ids, mi_stream_t stream) {
    int bad = check_text(pp, n, ids != nullptr);
    if (bad) return bad;
    const mi_text_columns& p = *pp;
    bad = check_text_grads(p, g_tables);
    if (bad) return bad;
    const int64_t n_pairs = n * p.n_text;
    if (n_pairs == 0) return 0;
    const int w4 = p.width / 4, lpr = lanes_per_row(w4);
    hipLaunchKernelGGL(text_clear_kernel, dim3(grid_for(n_pairs * lpr)), dim3(kBlock), 0, (hipStream_t)stream, n, n_pairs, w4, lpr, ids,
                       csr_of(p), grad_tables(p, g_tables));
    return mi_launch_status();
}

}  // extern "C"
