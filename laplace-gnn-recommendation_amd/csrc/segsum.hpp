// Sum of gradient rows by destination table row over a list of references, without atomics: the table gradients of
// PinSAGE's item feature projector (pinsage_proj.hip) and of its text columns (pinsage_text.hip).
//
// A reference is (key, r): key = (slot << shift) | row names the destination row of table `slot`, r the row of g to add (through
// the caller's term: as it is, or scaled).  One destination is referenced thousands of times from every workgroup of any
// row-parallel grid, so the caller writes its references in the order it wants the sums taken and this file does the rest:
//   1. a stable radix sort of the keys with r as payload: the references of a destination become one run, in the caller's order;
//   2. chunk_kernel: the sorted list is cut into chunks of 64 references, one lane group per chunk.  A run of equal keys inside
//      a chunk is summed from +0 in order (16 rows of g in flight) and stored to its table row by that group alone.  A run that
//      crosses chunk borders leaves one partial row per chunk: the chunk where it starts writes part_tail[chunk], every later
//      chunk it reaches writes part_head[chunk] (a chunk that lies wholly inside the run: from_prev wins over into_next);
//   3. combine_kernel: the group of the chunk where such a run starts adds part_tail[chunk] + part_head[chunk + 1] + ... in
//      chunk order and stores the row;
//   4. (callers that consume the sums at once) head_kernel: one lane group per reference; the group of the reference that heads
//      its run of equal keys hands the finished row to the caller's per-row operation — the lazy Adam update of
//      lazy_adam.hpp.  After the combine, because a run that crosses chunk borders is not complete before it.
// One writer per row and a fixed association that does not depend on scheduling: equal bits on every call
// (tests/segsum_emulation.py restates it).  The scheme of refsum.hpp (the LightGCN trainer's loss paths), with float4 lanes.
// The reference count is the host's n_ref, or min(*count, n_ref) read on the device when the caller counts its references
// there (slots past the count hold a key that sorts last and are never read).
#pragma once
#include "common.hpp"
#include <rocprim/rocprim.hpp>
#include <algorithm>

namespace segsum {

constexpr int kBlock = 256;
constexpr int kChunk = 64;       // references per chunk
constexpr int kInFlight = 16;    // rows of g a lane group keeps in flight

// lanes of the group that owns a chunk (or any row of w4 float4): a power of two >= w4
inline int lanes_per_row(int w4) {
    int l = 4;
    while (l < w4) l *= 2;
    return l;
}

template <typename T, int kSlots>
struct Ptrs {   // one pointer per slot, by value in the kernel arguments
    T* t[kSlots];
    __device__ __forceinline__ T* at(int slot) const {   // selects, no dynamically indexed copy of a kernel argument
        T* p = t[0];
#pragma unroll
        for (int s = 1; s < kSlots; ++s) p = (s == slot) ? t[s] : p;
        return p;
    }
};

// The per-reference term: what a chunk loads beside the row of g, and what it adds.  Plain: nothing, the row itself.
struct Plain {
    struct Loaded {};
    __device__ __forceinline__ Loaded load(uint64_t, uint32_t, unsigned) const { return {}; }
    __device__ __forceinline__ float4 apply(const float4& row, Loaded) const { return row; }
};

// One group of `lpr` lanes per chunk of 64 sorted references.
template <int kSlots, bool kDeviceCount, typename Term>
__global__ __launch_bounds__(kBlock) void chunk_kernel(int64_t n_ref_max, const int64_t* __restrict__ count, int w4, int lpr,
                                                       unsigned shift, const uint64_t* __restrict__ keys,
                                                       const uint32_t* __restrict__ refs, const float4* __restrict__ g, int64_t ldg4,
                                                       Term term, Ptrs<float4, kSlots> gt, float4* __restrict__ part_head,
                                                       float4* __restrict__ part_tail) {
    // A small launch is a handful of wavefronts walking 64 references each, one after the other: its time is the
    // instruction count per reference.  The table base comes from LDS (one read) instead of a select chain.
    __shared__ float4* tab[kSlots];
    if (threadIdx.x < kSlots) tab[threadIdx.x] = gt.at((int)threadIdx.x);
    __syncthreads();
    int64_t n_ref = n_ref_max;
    if constexpr (kDeviceCount) n_ref = min(*count, n_ref_max);
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
    // Two dependent loads per reference (its index, then its row of g and what the term loads): the indices and keys of step
    // s + 1 are fetched while the rows of step s are in flight, so a chunk costs one memory latency per step, not two.
    uint64_t kn[kInFlight + 1];
    uint32_t rn[kInFlight];
#pragma unroll
    for (int u = 0; u <= kInFlight; ++u) kn[u] = keys[j0 + min(u, n_here - 1)];
#pragma unroll
    for (int u = 0; u < kInFlight; ++u) rn[u] = refs[j0 + min(u, n_here - 1)];
    for (int q0 = 0; q0 < n_here; q0 += kInFlight) {
        uint64_t kq[kInFlight + 1];
        float4 rows[kInFlight];
        typename Term::Loaded extra[kInFlight];
#pragma unroll
        for (int u = 0; u <= kInFlight; ++u) kq[u] = kn[u];
#pragma unroll
        for (int u = 0; u < kInFlight; ++u) {
            rows[u] = g[(int64_t)rn[u] * ldg4 + e];
            extra[u] = term.load(kq[u], rn[u], shift);
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
            acc = mi_f4_add(acc, term.apply(rows[u], extra[u]));
            const bool last_of_run = (q + 1 == n_here) || kq[u + 1] != kq[u];
            if (!last_of_run) continue;
            const bool from_prev = run_start == 0 && head_open;
            const bool into_next = (q + 1 == n_here) && next_same;
            float4* dst;
            if (from_prev) dst = part_head + chunk * w4;          // finished by the chunk where the run starts
            else if (into_next) dst = part_tail + chunk * w4;     // this chunk starts the run; combine_kernel finishes it
            else dst = tab[kq[u] >> shift] + (int64_t)(kq[u] & mask) * w4;   // the row's only writer
            dst[e] = acc;
            acc = mi_f4_zero();
            run_start = q + 1;
        }
    }
}

// One lane group per chunk whose trailing run starts in it and runs on: tail partial + the head partials of the following
// chunks, in chunk order.
template <int kSlots, bool kDeviceCount>
__global__ __launch_bounds__(kBlock) void combine_kernel(int64_t n_ref_max, const int64_t* __restrict__ count, int w4, int lpr,
                                                         unsigned shift, const uint64_t* __restrict__ keys,
                                                         Ptrs<float4, kSlots> gt, const float4* __restrict__ part_head,
                                                         const float4* __restrict__ part_tail) {
    int64_t n_ref = n_ref_max;
    if constexpr (kDeviceCount) n_ref = min(*count, n_ref_max);
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
    gt.at((int)(key >> shift))[(int64_t)(key & mask) * w4 + e] = acc;
}

// One lane group per sorted reference; all but the group of a run's first reference leave at the head test (n_ref is at most a
// few times the rows of a block: a compaction of the heads would cost more than the idle groups).  op(slot, off, cell): cell
// is float4 `off` (= row * w4 + e) of table `slot`'s buffer, inside a summed row; each (slot, row) is seen by exactly one group.
template <int kSlots, bool kDeviceCount, typename RowOp>
__global__ __launch_bounds__(kBlock) void head_kernel(int64_t n_ref_max, const int64_t* __restrict__ count, int w4, int lpr,
                                                      unsigned shift, const uint64_t* __restrict__ keys, Ptrs<float4, kSlots> gt,
                                                      RowOp op) {
    int64_t n_ref = n_ref_max;
    if constexpr (kDeviceCount) n_ref = min(*count, n_ref_max);   // the slots past it hold the padding key: never a head
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t j = t / lpr;
    const int e = (int)(t - j * lpr);
    if (j >= n_ref || e >= w4) return;
    const uint64_t key = keys[j];
    if (j > 0 && keys[j - 1] == key) return;                     // not the head of its run
    const uint64_t mask = ((uint64_t)1 << shift) - 1;
    const int slot = (int)(key >> shift);
    const int64_t row = (int64_t)(key & mask);
    const int64_t off = row * w4 + e;
    op(slot, off, gt.at(slot) + off);
}

// ---- host ------------------------------------------------------------------------------------------------------------------
// The sort's double buffers (the caller writes its references to k0 / r0), rocprim's temporary storage (tmp_cap bytes: the
// caller's bound; it may use tmp itself before the sort) and one head and one tail partial row of `width` floats per chunk.
struct Buffers {
    uint64_t *k0, *k1;
    uint32_t *r0, *r1;
    char* tmp;
    size_t tmp_cap;
    float *part_head, *part_tail;
    bool ok() const { return k0 && k1 && r0 && r1 && tmp && part_head && part_tail; }
};

inline size_t workspace_bytes(int64_t n_ref, int width, size_t tmp_cap) {
    const size_t nr = (size_t)std::max<int64_t>(n_ref, 1), nc = (size_t)std::max<int64_t>(mi_ceil_div(n_ref, kChunk), 1);
    return 2 * mi_align_up(nr * sizeof(uint64_t), 256) + 2 * mi_align_up(nr * sizeof(uint32_t), 256) + mi_align_up(tmp_cap, 256) +
           2 * mi_align_up(nc * width * sizeof(float), 256);
}

inline Buffers take(MiArena& arena, int64_t n_ref, int width, size_t tmp_cap) {
    const size_t nr = (size_t)std::max<int64_t>(n_ref, 1), nc = (size_t)std::max<int64_t>(mi_ceil_div(n_ref, kChunk), 1);
    Buffers b;
    b.k0 = arena.take<uint64_t>(nr);
    b.k1 = arena.take<uint64_t>(nr);
    b.r0 = arena.take<uint32_t>(nr);
    b.r1 = arena.take<uint32_t>(nr);
    b.tmp_cap = tmp_cap;
    b.tmp = arena.take<char>(tmp_cap);
    b.part_head = arena.take<float>(nc * width);
    b.part_tail = arena.take<float>(nc * width);
    return b;
}

// n_ref > 0 references of `bits` key bits.  The sort's size query enqueues nothing; MI_ERR_WORKSPACE when rocprim's need, or
// other_tmp_need (what the caller found it needs of tmp itself), exceeds tmp_cap.  Only then build_refs() (-> 0 or an error
// code) enqueues what writes k0 / r0 (and *count), and the sort, the chunks and the combine follow.  sorted_keys (optional):
// which of k0 / k1 holds the sorted keys afterwards (for run_heads).
template <bool kDeviceCount, int kSlots, typename Term, typename BuildRefs>
int run(const Buffers& b, int64_t n_ref, const int64_t* count, unsigned shift, unsigned bits, size_t other_tmp_need,
        BuildRefs&& build_refs, const float* g, int64_t ldg, int width, Term term, const Ptrs<float4, kSlots>& gt, hipStream_t s,
        const uint64_t** sorted_keys = nullptr) {
    rocprim::double_buffer<uint64_t> keys(b.k0, b.k1);
    rocprim::double_buffer<uint32_t> refs(b.r0, b.r1);
    size_t need = 0;
    MI_HIP(rocprim::radix_sort_pairs(nullptr, need, keys, refs, (size_t)n_ref, 0u, bits, s));
    if (other_tmp_need > b.tmp_cap || need > b.tmp_cap) return MI_ERR_WORKSPACE;
    // ---- nothing has been enqueued up to here ----
    const int rc = build_refs();
    if (rc) return rc;
    MI_HIP(rocprim::radix_sort_pairs(b.tmp, need, keys, refs, (size_t)n_ref, 0u, bits, s));
    const int w4 = width / 4, lpr = lanes_per_row(w4);
    const dim3 grid((unsigned)mi_ceil_div(mi_ceil_div(n_ref, kChunk) * lpr, kBlock));
    hipLaunchKernelGGL((chunk_kernel<kSlots, kDeviceCount, Term>), grid, dim3(kBlock), 0, s, n_ref, count, w4, lpr, shift,
                       (const uint64_t*)keys.current(), (const uint32_t*)refs.current(), reinterpret_cast<const float4*>(g), ldg / 4,
                       term, gt, reinterpret_cast<float4*>(b.part_head), reinterpret_cast<float4*>(b.part_tail));
    hipLaunchKernelGGL((combine_kernel<kSlots, kDeviceCount>), grid, dim3(kBlock), 0, s, n_ref, count, w4, lpr, shift,
                       (const uint64_t*)keys.current(), gt, reinterpret_cast<const float4*>(b.part_head),
                       reinterpret_cast<const float4*>(b.part_tail));
    if (sorted_keys) *sorted_keys = keys.current();
    return mi_launch_status();
}

// op on every summed row of the run() that left `keys` (same n_ref, count, shift, width, gt), after its combine.
template <bool kDeviceCount, int kSlots, typename RowOp>
int run_heads(const uint64_t* keys, int64_t n_ref, const int64_t* count, unsigned shift, int width, const Ptrs<float4, kSlots>& gt,
              RowOp op, hipStream_t s) {
    const int w4 = width / 4, lpr = lanes_per_row(w4);
    const dim3 grid((unsigned)mi_ceil_div(n_ref * lpr, kBlock));
    hipLaunchKernelGGL((head_kernel<kSlots, kDeviceCount, RowOp>), grid, dim3(kBlock), 0, s, n_ref, count, w4, lpr, shift, keys, gt, op);
    return mi_launch_status();
}

}  // namespace segsum
