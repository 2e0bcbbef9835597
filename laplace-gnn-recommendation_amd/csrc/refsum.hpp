// Sum of weighted source rows by destination row over a list of references, without float atomics: the end of every loss
// path of the LightGCN trainer (train.hip: bpr_chunk_kernel, rank_chunk_kernel; inbatch.hip, contrastive.hip and
// fullsoftmax.hip: their chunk kernels).
//
// A reference is (key, r): key names the destination row of g_final, r is the caller's (what it adds is the caller's term
// list: source rows and weights).  The caller writes keys and references in the order it wants the sums taken; then
//   1. a stable radix sort of the keys with r as payload: the references of a row become one run, in the caller's order;
//   2. the caller's chunk kernel: the sorted list is cut into chunks of 64, one wavefront each, lane L holding reference
//      j0 + L.  A run of equal keys inside a chunk is summed from +0 in order (8 source rows in flight) and stored to its row by
//      that wavefront alone.  A run that crosses chunk borders leaves one partial row per chunk (RunWriter::close);
//   3. combine_kernel: the wavefront of the chunk where such a run starts adds its partial rows in chunk order and stores the row;
//   4. finish_kernel: the per-slot loss terms and L2 terms become the loss, one block, fixed order.
// The run lengths also give the L2 weight of every node of the batch (run_length): one writer per entry.
// One writer per row and fixed orders throughout: the whole train step is bitwise reproducible.
// Scalar lanes (a lane holds floats lane, lane + 64, ... of a row: VPT = ceil(d / 64) of them) and 32-bit keys; segsum.hpp is
// the same scheme for float4 lane groups, 64-bit slot keys and a device-side count.
#pragma once
#include "common.hpp"
#include <rocprim/rocprim.hpp>

namespace refsum {

constexpr int kBlock = 256;
constexpr int kChunk = 64;      // references per chunk: one per lane
constexpr int kInFlight = 8;    // source rows a wavefront keeps in flight

// f(std::integral_constant<int, N>), N = 1, 2, 4 or 8 >= n (the floats of a row per lane, VPT; 32-column tiles of a row)
template <class F>
void with_vpt(int64_t n, F&& f) {
    if (n <= 1) f(std::integral_constant<int, 1>{});
    else if (n <= 2) f(std::integral_constant<int, 2>{});
    else if (n <= 4) f(std::integral_constant<int, 4>{});
    else f(std::integral_constant<int, 8>{});
}

// ---- device pieces: registers only (no LDS, every array index a constant after unrolling) -----------------------------------
struct Chunk {
    int64_t id, j0;               // the chunk of this wavefront; its first reference
    int n_here, lane;             // references in the chunk (0: the chunk lies past the list); this lane
    uint32_t key;                 // key of reference j0 + lane (0xFFFFFFFF on the lanes past n_here)
    bool head_open, next_same;    // the first run began in an earlier chunk; the last run goes on in the next
};

__device__ __forceinline__ Chunk open_chunk(const uint32_t* __restrict__ keys, int64_t n_ref) {
    Chunk c;
    c.id = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / MI_WAVE;
    c.j0 = c.id * kChunk;
    c.lane = mi_lane();
    c.n_here = 0;
    c.key = 0xFFFFFFFFu;
    c.head_open = c.next_same = false;
    if (c.j0 >= n_ref) return c;
    c.n_here = (int)min((int64_t)kChunk, n_ref - c.j0);
    if (c.lane < c.n_here) c.key = keys[c.j0 + c.lane];
    // The four border keys by loads of their own at clamped positions, no shuffle of c.key and no branch: they are in flight
    // beside whatever the caller loads next and are waited for where a run closes, not here.
    const int64_t j_end = c.j0 + c.n_here;
    const uint32_t before = keys[max(c.j0 - 1, (int64_t)0)], first = keys[c.j0];
    const uint32_t last = keys[j_end - 1], after = keys[min(j_end, n_ref - 1)];
    c.head_open = (c.j0 > 0) & (before == first);
    c.next_same = (j_end < n_ref) & (after == last);
    return c;
}

// Length of the run of equal keys that reference j opens, 0 when j does not open its run: the opening reference finds the run's
// end by bisection.  The L2 weight of the run's node is (its references in the batch) x (one reference's share), so the caller
// stores reg_w[node] = (float)length * reg_unit and is the entry's only writer (reg_w is zero on entry).
__device__ __forceinline__ int64_t run_length(const uint32_t* __restrict__ keys, int64_t j, int64_t n_ref) {
    const uint32_t key = keys[j];
    if (j > 0 && keys[j - 1] == key) return 0;
    int64_t lo = j + 1, hi = n_ref;   // first position in (j, n_ref] whose key differs
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[mid] == key) lo = mid + 1; else hi = mid;
    }
    return lo - j;
}

struct Dest {   // where the sums go: rows of g_final, and one head and one tail partial row of d floats per chunk
    float* __restrict__ g_final;
    int64_t ldg;
    float* __restrict__ part_head;
    float* __restrict__ part_tail;
    int d;
    bool add = false;   // the finished rows are ADDED to what g_final holds (still one writer per row) instead of stored
};

// The sum of the run a wavefront is in, and where it goes when the run closes.
template <int VPT>
struct RunWriter {
    float acc[VPT];
    int run_start = 0;   // first reference (within the chunk) of the run being summed
    __device__ __forceinline__ RunWriter() {
#pragma unroll
        for (int v = 0; v < VPT; ++v) acc[v] = 0.f;
    }
    __device__ __forceinline__ void add(float w, const float (&x)[VPT]) {
#pragma unroll
        for (int v = 0; v < VPT; ++v) acc[v] = fmaf(w, x[v], acc[v]);
    }
    // After the last term of reference q (wave-uniform).  Nothing happens unless q ends its run within the chunk.  A run that
    // came in from the previous chunk goes to part_head[chunk], also when it runs on into the next one: a chunk that lies
    // wholly inside a run is a head partial, from_prev wins over into_next, and the combine walks head partials until a
    // chunk's last key differs.  A run that starts here and runs on goes to part_tail[chunk]; a run inside the chunk goes
    // to its row of g_final, whose only writer this wavefront is (g_final is zero on entry: a store, no read-modify-write;
    // with Dest::add the row is added to what g_final holds instead, for a caller whose table another loss has filled).
    __device__ __forceinline__ void close(const Chunk& c, int q, const Dest& to) {
        const uint32_t kq = __shfl(c.key, q, MI_WAVE);
        const bool last_of_run = (q + 1 == c.n_here) || __shfl(c.key, q + 1, MI_WAVE) != kq;
        if (!last_of_run) return;
        const bool from_prev = run_start == 0 && c.head_open;
        const bool into_next = (q + 1 == c.n_here) && c.next_same;
        float* dst;
        if (from_prev) dst = to.part_head + c.id * to.d;         // finished by the chunk where the run starts
        else if (into_next) dst = to.part_tail + c.id * to.d;    // this chunk starts the run; combine_kernel finishes it
        else dst = to.g_final + (int64_t)kq * to.ldg;
        const bool add = to.add && !from_prev && !into_next;   // partial rows are always stored
#pragma unroll
        for (int v = 0; v < VPT; ++v) {
            const int k = c.lane + v * MI_WAVE;
            if (k < to.d) dst[k] = add ? dst[k] + acc[v] : acc[v];
            acc[v] = 0.f;
        }
        run_start = q + 1;
    }
};

// The in-order pass of a chunk whose references carry at most Term::kTerms terms each, held by the reference's own lane:
// kInFlight references' source rows in flight together.  Term says, by shuffle from lane q,
//   row(t, q)      the row of `rows` that term t of reference q adds
//   weight(t, q)   its weight; term 0 always counts, a later term only where its weight is not zero (wave-uniform)
// A constant weight of 1 makes the fmaf a plain addition, bit for bit.
template <int VPT, class Term>
__device__ __forceinline__ void walk_references(const Chunk& c, const Term& term, const float* __restrict__ rows, int64_t ld,
                                                const Dest& to) {
    RunWriter<VPT> run;
    for (int q0 = 0; q0 < c.n_here; q0 += kInFlight) {
        float x[kInFlight][Term::kTerms][VPT], w[kInFlight][Term::kTerms];
#pragma unroll
        for (int u = 0; u < kInFlight; ++u) {
            const int q = min(q0 + u, c.n_here - 1);
            const bool live = q0 + u < c.n_here;
#pragma unroll
            for (int t = 0; t < Term::kTerms; ++t) {
                w[u][t] = term.weight(t, q);
                const float* row = rows + term.row(t, q) * ld;
                const bool read = live && (t == 0 || w[u][t] != 0.f);
#pragma unroll
                for (int v = 0; v < VPT; ++v) {
                    const int k = c.lane + v * MI_WAVE;
                    x[u][t][v] = (read && k < to.d) ? row[k] : 0.f;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kInFlight; ++u) {
            const int q = q0 + u;
            if (q >= c.n_here) break;
#pragma unroll
            for (int t = 0; t < Term::kTerms; ++t)
                if (t == 0 || w[u][t] != 0.f) run.add(w[u][t], x[u][t]);
            run.close(c, q, to);
        }
    }
}

// The Term of a reference that adds one row as it stands: row `src` of `rows`, unweighted.
struct SlotRow {
    static constexpr int kTerms = 1;
    int64_t src = 0;
    __device__ __forceinline__ int64_t row(int, int q) const { return __shfl(src, q, MI_WAVE); }
    __device__ __forceinline__ float weight(int, int) const { return 1.f; }
};

// ---- kernels ----------------------------------------------------------------------------------------------------------------
// One wavefront per chunk whose trailing run starts in it and runs on: tail partial + the head partials of the following
// chunks, in chunk order, stored to the row.
template <int VPT>
static __global__ __launch_bounds__(kBlock) void combine_kernel(int64_t n_ref, int d, const uint32_t* __restrict__ keys,
                                                                const float* __restrict__ part_head,
                                                                const float* __restrict__ part_tail,
                                                                float* __restrict__ g_final, int64_t ldg, bool add) {
    const int64_t chunk = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / MI_WAVE;
    const int64_t j0 = chunk * kChunk;
    if (j0 >= n_ref) return;
    const int64_t j_last = min(j0 + kChunk, n_ref) - 1;
    if (j_last + 1 >= n_ref) return;                       // nothing after this chunk
    const uint32_t row = keys[j_last];
    if (keys[j_last + 1] != row) return;                   // the trailing run ends here
    if (keys[j0] == row && j0 > 0 && keys[j0 - 1] == row) return;  // the run started in an earlier chunk: not the owner
    const int lane = mi_lane();
    float acc[VPT];
#pragma unroll
    for (int v = 0; v < VPT; ++v) {
        const int k = lane + v * MI_WAVE;
        acc[v] = k < d ? part_tail[chunk * d + k] : 0.f;
    }
    for (int64_t nb = chunk + 1; nb * kChunk < n_ref && keys[nb * kChunk] == row; ++nb) {
#pragma unroll
        for (int v = 0; v < VPT; ++v) {
            const int k = lane + v * MI_WAVE;
            if (k < d) acc[v] += part_head[nb * d + k];
        }
        if (keys[min((nb + 1) * kChunk, n_ref) - 1] != row) break;   // the run ends inside chunk nb
    }
    float* dst = g_final + (int64_t)row * ldg;
#pragma unroll
    for (int v = 0; v < VPT; ++v) {
        const int k = lane + v * MI_WAVE;
        if (k < d) dst[k] = add ? dst[k] + acc[v] : acc[v];
    }
}

// Single block, fixed order: loss = mean_scale * sum(term) + lambda * sum(reg).  mean_scale is the signed 1 / count: the callers
// whose slot terms are stored negated pass -1 / count.
static __global__ __launch_bounds__(1024) void finish_kernel(int64_t batch, const float* __restrict__ term_v,
                                                             const float* __restrict__ reg_v, float mean_scale, float lambda,
                                                             float* __restrict__ loss_out) {
    __shared__ float sh_a[1024];
    __shared__ float sh_b[1024];
    const int t = threadIdx.x;
    float a = 0.f, r = 0.f;
#pragma unroll 4
    for (int64_t i = t; i < batch; i += 1024) {   // coalesced, independent loads (a contiguous slice per thread was a chain
        a += term_v[i];                            // of 16 strided loads: 17 us at B = 16 384); fixed order all the same
        r += reg_v[i];
    }
    sh_a[t] = a;
    sh_b[t] = r;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if (t < s) {
            sh_a[t] += sh_a[t + s];
            sh_b[t] += sh_b[t + s];
        }
        __syncthreads();
    }
    if (t == 0) loss_out[0] = sh_a[0] * mean_scale + lambda * sh_b[0];
}

// ---- host -------------------------------------------------------------------------------------------------------------------
// The sort's double buffers (the caller's reference kernel writes k0 / r0), rocprim's temporary storage and one head and one
// tail partial row of part_width floats per chunk.
struct Buffers {
    uint32_t *k0, *k1, *r0, *r1;
    char* tmp;
    size_t tmp_cap;
    float *part_head, *part_tail;
    bool ok() const { return k0 && k1 && r0 && r1 && tmp && part_head && part_tail; }
};

// bound of rocprim's temporary storage for a sort of n_ref (key, reference) pairs; a multiple of 256
inline size_t tmp_bytes(int64_t n_ref) { return ((size_t)1 << 20) + mi_align_up((size_t)n_ref * 2, 256); }

inline size_t workspace_bytes(int64_t n_ref, int64_t part_width) {
    const size_t chunks = (size_t)mi_ceil_div(n_ref, kChunk);
    return 4 * mi_align_up((size_t)n_ref * sizeof(uint32_t), 256) + tmp_bytes(n_ref) +
           2 * mi_align_up(chunks * (size_t)part_width * sizeof(float), 256);
}

inline Buffers take(MiArena& arena, int64_t n_ref, int64_t part_width) {
    const size_t chunks = (size_t)mi_ceil_div(n_ref, kChunk);
    Buffers b;
    b.k0 = arena.take<uint32_t>(n_ref);
    b.k1 = arena.take<uint32_t>(n_ref);
    b.r0 = arena.take<uint32_t>(n_ref);
    b.r1 = arena.take<uint32_t>(n_ref);
    b.tmp_cap = tmp_bytes(n_ref);
    b.tmp = arena.take<char>(b.tmp_cap);
    b.part_head = arena.take<float>(chunks * (size_t)part_width);
    b.part_tail = arena.take<float>(chunks * (size_t)part_width);
    return b;
}

// The sort of n_ref references, planned before anything is enqueued and run after the caller's reference kernel.
struct Sort {
    rocprim::double_buffer<uint32_t> keys, refs;
    unsigned bits;
    size_t need;
};

// compact: the keys are slots of a batch-node map, all < n_ref; node ids otherwise, which need all 32 bits.  The size query
// enqueues nothing: MI_ERR_WORKSPACE comes back with the stream as it was.
inline int plan_sort(const Buffers& b, int64_t n_ref, bool compact, hipStream_t s, Sort& plan) {
    plan.keys = rocprim::double_buffer<uint32_t>(b.k0, b.k1);
    plan.refs = rocprim::double_buffer<uint32_t>(b.r0, b.r1);
    plan.bits = compact ? mi_bits_for(n_ref) : 32;
    plan.need = 0;
    MI_HIP(rocprim::radix_sort_pairs(nullptr, plan.need, plan.keys, plan.refs, (size_t)n_ref, 0, plan.bits, s));
    return plan.need > b.tmp_cap ? MI_ERR_WORKSPACE : 0;
}

// afterwards plan.keys.current() / plan.refs.current() hold the sorted list
inline int sort(const Buffers& b, int64_t n_ref, hipStream_t s, Sort& plan) {
    MI_HIP(rocprim::radix_sort_pairs(b.tmp, plan.need, plan.keys, plan.refs, (size_t)n_ref, 0, plan.bits, s));
    return 0;
}

// grid of a kernel with one wavefront per chunk
inline dim3 chunk_grid(int64_t n_ref) { return dim3((unsigned)mi_ceil_div(mi_ceil_div(n_ref, kChunk) * MI_WAVE, kBlock)); }

template <int VPT>
void launch_combine(const Sort& plan, int64_t n_ref, const Dest& to, hipStream_t s) {
    hipLaunchKernelGGL(combine_kernel<VPT>, chunk_grid(n_ref), dim3(kBlock), 0, s, n_ref, to.d, (const uint32_t*)plan.keys.current(),
                       (const float*)to.part_head, (const float*)to.part_tail, to.g_final, to.ldg, to.add);
}

inline void launch_finish(int64_t batch, const float* term_v, const float* reg_v, float mean_scale, float lambda,
                          float* loss_out, hipStream_t s) {
    hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(1024), 0, s, batch, term_v, reg_v, mean_scale, lambda, loss_out);
}

}  // namespace refsum
