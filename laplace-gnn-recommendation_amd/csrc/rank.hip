// K10r: the full-catalogue rank of one target item per query row — how many admissible items beat it, in the order top-K
// uses (score desc, item id asc).  Where K10 selects the k best of a row, this counts: no threshold sample, no candidate
// lists, no sort, no fallback rows.  The output is an integer, every sum is an integer sum: exact and reproducible.
//
//   1. rank_target_kernel: s_t of every row by the scalar fma chain (the same bits as the MFMA and the GEMM), the target as
//      int32 (-1: outside [0, n_items)), rank[p] = 0.
//   2. every item is counted, exclusions or not:
//      path F (fused-eligible tables, include/laplace_hip.h)  rank_count_fused_kernel: a workgroup owns a 64-query panel and a
//        slice of 64-item tiles, as topk_scores_filter_kernel does; the 16 accumulator values of a lane are compared with
//        their rows' (s_t, t), held in registers, and added to 16 integer counters that live in registers for the whole
//        slice; one integer atomicAdd per row and workgroup at the end of the slice.
//      path M (every other layout or width)  the score block through mi_gemm_launch, as K10's path M, then
//        rank_count_rows_kernel, one workgroup per row, which also takes s_t from the block.
//   3. rank_exclusions_kernel, one workgroup per row, off the hot loop: one pass over the row's exclusion list; an
//      atomicOr into the row's bitmap tells the first occurrence of an id; first occurrences are counted (n_excluded), one
//      equal to t marks the row -1, any other is scored (fma chain / read from the block) and takes one off the count if it
//      beats t.  The same kernel ends the rows whose target is out of range (-1) when there are no exclusions at all.
// The compares are float compares: for finite scores s > s_t <=> key(s) > key(s_t) and s == s_t <=> the keys are equal
// (score_key sends -0 to +0, and -0 == +0); non-finite embeddings are outside the contract, as for K10.
#include "gemm.hpp"
#include "score_panel.hpp"

namespace {

constexpr int kBlock = 256;

__device__ __forceinline__ bool beats(float s, int32_t j, float st, int32_t t) {
    return s > st || (s == st && j < t);
}

__device__ __forceinline__ float fma_chain(const float* __restrict__ u, const float* __restrict__ it, int d) {
    float acc = 0.f;
    for (int c = 0; c < d; ++c) acc = fmaf(u[c], it[c], acc);
    return acc;
}

__global__ __launch_bounds__(kBlock) void rank_target_kernel(int64_t n_q, int64_t n_items, int d,
                                                             const int64_t* __restrict__ uid,
                                                             const int64_t* __restrict__ target,
                                                             const float* __restrict__ U, int64_t ldu,
                                                             const float* __restrict__ I, int64_t ldi,
                                                             float* __restrict__ st, int32_t* __restrict__ tt,
                                                             int32_t* __restrict__ rank, float* __restrict__ out_score) {
    const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (q >= n_q) return;
    const int64_t t = target[q];
    const bool ok = t >= 0 && t < n_items;
    const float s = ok ? fma_chain(U + uid[q] * ldu, I + t * ldi, d) : 0.f;
    st[q] = ok ? s : INFINITY;   // no finite score beats it: such a row counts nothing
    tt[q] = ok ? (int32_t)t : -1;
    rank[q] = 0;
    if (out_score) out_score[q] = s;
}

struct RankArgs {
    int64_t n_q, n_items;
    int d;
    const int64_t* uid;
    const float* U; int64_t ldu;
    const float* I; int64_t ldi;
    const float* st;            // [n_q] target scores
    const int32_t* tt;          // [n_q] targets, -1 = none
    int32_t* rank;              // [n_q], zeroed
    int64_t tiles_per_slice;    // item panels per workgroup along blockIdx.x
};

// Path F.  The tile loop is topk_scores_filter_kernel's: the query panel and the current item panel in LDS, the next item
// panel's global loads in flight under the MFMA chain, one accumulator, k ascending.  The epilogue touches no memory at
// all; two workgroups per CU, so one wavefront's compares run beside the other's MFMA chain on the same SIMD.
__global__ __launch_bounds__(256, 2) void rank_count_fused_kernel(RankArgs a) {
    __shared__ float As[FM][FKPAD];
    __shared__ float Bs[FN][FKPAD];
    __shared__ int red[FM];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const int64_t m0 = (int64_t)blockIdx.y * FM;
    const int64_t n_tiles = (a.n_items + FN - 1) / FN;
    const int64_t t0 = (int64_t)blockIdx.x * a.tiles_per_slice;
    const int64_t t1 = min(n_tiles, t0 + a.tiles_per_slice);
    if (t0 >= t1) return;
    float4 va[8], vb[8];
    fpanel_issue(va, a.U, a.ldu, a.uid, m0, a.n_q, a.d, tid);
    fpanel_issue(vb, a.I, a.ldi, nullptr, t0 * FN, a.n_items, a.d, tid);
    fpanel_commit(As, va, tid);
    fpanel_commit(Bs, vb, tid);
    if (tid < FM) red[tid] = 0;
    // this lane's 16 accumulator rows are fixed for the whole launch: their targets live in registers
    // (rows beyond n_q: +inf / -1 count nothing, and are not written either)
    float st[16];
    int32_t tt[16];
    int cnt[16];
    const int row_base = wm * 32 + 4 * (lane >> 5);
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int64_t gm = m0 + row_base + (reg & 3) + 8 * (reg >> 2);
        st[reg] = gm < a.n_q ? a.st[gm] : INFINITY;
        tt[reg] = gm < a.n_q ? a.tt[gm] : -1;
        cnt[reg] = 0;
    }
    __syncthreads();
    const float* ap = &As[wm * 32 + (lane & 31)][lane >> 5];
    const float* bp = &Bs[wn * 32 + (lane & 31)][lane >> 5];
    const int n_mfma = (a.d + 1) / 2;  // the panels are zero beyond d
    for (int64_t t = t0; t < t1; ++t) {
        const bool more = t + 1 < t1;
        if (more) fpanel_issue(vb, a.I, a.ldi, nullptr, (t + 1) * FN, a.n_items, a.d, tid);  // in flight under the MFMAs
        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
        if (n_mfma == FKC / 2) {
#pragma unroll 64
            for (int s = 0; s < FKC / 2; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[2 * s], bp[2 * s], acc, 0, 0, 0);
        } else if (n_mfma == FKC / 4) {
#pragma unroll 32
            for (int s = 0; s < FKC / 4; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[2 * s], bp[2 * s], acc, 0, 0, 0);
        } else {
            for (int s = 0; s < n_mfma; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[2 * s], bp[2 * s], acc, 0, 0, 0);
        }
        const int64_t gn = t * FN + wn * 32 + (lane & 31);
        if (gn < a.n_items) {   // the zero rows that pad the last panel score 0: they are no items
            const int32_t j = (int32_t)gn;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) cnt[reg] += beats(acc[reg], j, st[reg], tt[reg]) ? 1 : 0;
        }
        __syncthreads();  // every wavefront is done reading Bs
        if (more) {
            fpanel_commit(Bs, vb, tid);
            __syncthreads();
        }
    }
    // the 32 lanes that share a row, then the two item-side wavefronts (LDS), then one atomic per row
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        int v = cnt[reg];
#pragma unroll
        for (int off = 16; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        if ((lane & 31) == 0 && v) atomicAdd(&red[row_base + (reg & 3) + 8 * (reg >> 2)], v);
    }
    __syncthreads();
    if (tid < FM && m0 + tid < a.n_q && red[tid]) atomicAdd(&a.rank[m0 + tid], red[tid]);
}

// Path M: one workgroup per row of the materialised score block (rows q0 .. q0 + n_rows of the call).
__global__ __launch_bounds__(kBlock) void rank_count_rows_kernel(int64_t n_items, const float* __restrict__ scores,
                                                                 float* __restrict__ st, const int32_t* __restrict__ tt,
                                                                 int32_t* __restrict__ rank, float* __restrict__ out_score) {
    __shared__ int red;
    const int64_t q = blockIdx.x;
    const float* row = scores + q * n_items;
    const int32_t t = tt[q];
    if (threadIdx.x == 0) red = 0;
    __syncthreads();
    if (t < 0) return;   // block-uniform; rank_exclusions_kernel writes the -1
    const float s_t = row[t];
    int c = 0;
    for (int64_t i = threadIdx.x; i < n_items; i += kBlock) c += beats(row[i], (int32_t)i, s_t, t) ? 1 : 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&red, c);
    __syncthreads();
    if (threadIdx.x == 0) {
        rank[q] = red;
        st[q] = s_t;
        if (out_score) out_score[q] = s_t;
    }
}

// One workgroup per row.  scores: the row's materialised scores (path M, leading dimension n_items) or null (fma chain).
__global__ __launch_bounds__(kBlock) void rank_exclusions_kernel(RankArgs a, const int32_t* __restrict__ excl_ptr,
                                                                 const int32_t* __restrict__ excl_idx,
                                                                 uint32_t* __restrict__ bitmap, int64_t words,
                                                                 const float* __restrict__ scores,
                                                                 int32_t* __restrict__ n_excluded) {
    __shared__ int s_dec, s_nex, s_hit;
    const int64_t q = blockIdx.x;
    if (threadIdx.x == 0) { s_dec = 0; s_nex = 0; s_hit = 0; }
    __syncthreads();
    const int32_t t = a.tt[q];
    if (excl_ptr) {
        const float s_t = a.st[q];
        const float* u = a.U + a.uid[q] * a.ldu;
        int dec = 0, nex = 0;
        for (int32_t p = excl_ptr[q] + threadIdx.x; p < excl_ptr[q + 1]; p += kBlock) {
            const int32_t i = excl_idx[p];
            if (i < 0 || i >= a.n_items) continue;
            const uint32_t bit = 1u << (i & 31);
            if (atomicOr(&bitmap[q * words + (i >> 5)], bit) & bit) continue;   // a repeat of an id already seen
            ++nex;
            if (t < 0) continue;
            if (i == t) { s_hit = 1; continue; }
            const float s = scores ? scores[q * a.n_items + i] : fma_chain(u, a.I + (int64_t)i * a.ldi, a.d);
            dec += beats(s, i, s_t, t) ? 1 : 0;
        }
        if (dec) atomicAdd(&s_dec, dec);
        if (nex) atomicAdd(&s_nex, nex);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (t < 0 || s_hit) a.rank[q] = -1;
        else if (s_dec) a.rank[q] -= s_dec;
        if (n_excluded) n_excluded[q] = s_nex;
    }
}

}  // namespace

// The one decision of which path a call takes: the dispatcher and mi_rank_path both ask here.  K10's fused-eligible rule
// without its catalogue size: counting has no small-catalogue problem.
static int rank_choose_path(int64_t d, const float* user_emb, int64_t ldu, const float* item_emb, int64_t ldi) {
    const bool fused = d <= FKC && d % 4 == 0 && ldu % 4 == 0 && ldi % 4 == 0 && mi_aligned16(user_emb) && mi_aligned16(item_emb);
    return fused ? MI_RANK_PATH_FUSED : MI_RANK_PATH_MATERIALISED;
}

extern "C" {

int mi_rank_path(int64_t n_items, int64_t d, const float* user_emb, int64_t ldu, const float* item_emb, int64_t ldi) {
    MI_CHECK_ARG(n_items >= 0 && d > 0);
    if (n_items >= INT32_MAX) return MI_ERR_TOO_LARGE;
    MI_CHECK_ARG(user_emb && item_emb && ldu >= d && ldi >= d);
    return rank_choose_path(d, user_emb, ldu, item_emb, ldi);
}

size_t mi_rank_items_workspace_bytes(int64_t n_q, int64_t n_items) {
    if (n_q <= 0) return 256;
    if (n_items < 0) n_items = 0;
    const size_t words = (size_t)((n_items + 31) / 32);
    return mi_align_up((size_t)n_q * (size_t)n_items * sizeof(float), 256) +   // path M's score block (address space on path F)
           2 * mi_align_up((size_t)n_q * sizeof(float), 256) +                 // target scores, targets
           mi_align_up((size_t)n_q * words * sizeof(uint32_t), 256);           // exclusion bitmap
}

int mi_rank_items_f32(int64_t n_q, int64_t n_items, int64_t d, const int64_t* uid, const int64_t* target,
                      const float* user_emb, int64_t ldu, const float* item_emb, int64_t ldi,
                      const int32_t* excl_ptr, const int32_t* excl_idx, int32_t* out_rank, float* out_score,
                      int32_t* out_n_excluded, void* ws, size_t ws_bytes, mi_stream_t stream) {
    MI_CHECK_ARG(n_q >= 0 && n_items >= 0 && d > 0);
    if (n_q == 0) return 0;
    if (n_items >= INT32_MAX || mi_ceil_div(n_q, FM) > 65535 || d >= INT32_MAX) return MI_ERR_TOO_LARGE;   // grid.y: 64-row panels
    MI_CHECK_ARG(uid && target && user_emb && item_emb && out_rank && ws && ldu >= d && ldi >= d);
    // excl_idx may be null when every exclusion row is empty (excl_ptr all equal)
    if (ws_bytes < mi_rank_items_workspace_bytes(n_q, n_items)) return MI_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int64_t words = (n_items + 31) / 32;
    MiArena ar(ws, ws_bytes);
    float* scores = ar.take<float>((size_t)n_q * (size_t)n_items);
    float* st = ar.take<float>((size_t)n_q);
    int32_t* tt = ar.take<int32_t>((size_t)n_q);
    uint32_t* bitmap = ar.take<uint32_t>((size_t)n_q * (size_t)words);
    if (!scores || !st || !tt || !bitmap) return MI_ERR_WORKSPACE;
    hipLaunchKernelGGL(rank_target_kernel, dim3((unsigned)mi_ceil_div(n_q, kBlock)), dim3(kBlock), 0, s, n_q, n_items, (int)d,
                       uid, target, user_emb, ldu, item_emb, ldi, st, tt, out_rank, out_score);
    if (excl_ptr && n_items > 0) MI_HIP(hipMemsetAsync(bitmap, 0, (size_t)n_q * (size_t)words * sizeof(uint32_t), s));
    RankArgs a;
    a.n_q = n_q; a.n_items = n_items; a.d = (int)d; a.uid = uid;
    a.U = user_emb; a.ldu = ldu; a.I = item_emb; a.ldi = ldi;
    a.st = st; a.tt = tt; a.rank = out_rank; a.tiles_per_slice = 0;
    if (n_items == 0) {   // every target is out of range
        hipLaunchKernelGGL(rank_exclusions_kernel, dim3((unsigned)n_q), dim3(kBlock), 0, s, a, (const int32_t*)nullptr,
                           (const int32_t*)nullptr, bitmap, words, (const float*)nullptr, out_n_excluded);
        return mi_launch_status();
    }
    if (rank_choose_path(d, user_emb, ldu, item_emb, ldi) == MI_RANK_PATH_FUSED) {
        const int64_t strips = mi_ceil_div(n_q, FM), n_tiles = mi_ceil_div(n_items, FN);
        // the grid rule of K10's fused kernel: rounds of 2 workgroups per CU x (panels of a slice + the query-panel prologue)
        const int64_t capacity = 2 * (int64_t)mi_cu_count();
        int64_t slices = 1, best = INT64_MAX;
        for (int64_t l = 1; l <= n_tiles && l <= 4096; ++l) {
            const int64_t cost = mi_ceil_div(strips * l, capacity) * (mi_ceil_div(n_tiles, l) + 2);
            if (cost < best) { best = cost; slices = l; }
        }
        a.tiles_per_slice = mi_ceil_div(n_tiles, slices);
        slices = mi_ceil_div(n_tiles, a.tiles_per_slice);
        hipLaunchKernelGGL(rank_count_fused_kernel, dim3((unsigned)slices, (unsigned)strips), dim3(256), 0, s, a);
        hipLaunchKernelGGL(rank_exclusions_kernel, dim3((unsigned)n_q), dim3(kBlock), 0, s, a, excl_ptr, excl_idx, bitmap, words,
                           (const float*)nullptr, out_n_excluded);
        return mi_launch_status();
    }
    MiGemmArgs g{};
    g.M = n_q; g.N = n_items; g.K = d;
    g.A = user_emb; g.sa_m = ldu; g.sa_k = 1; g.a_rows = uid;
    g.B = item_emb; g.sb_n = ldi; g.sb_k = 1;
    g.bias = nullptr; g.C = scores; g.ldc = n_items; g.accumulate = 0; g.act = 0;
    const int rc = mi_gemm_launch(g, nullptr, 0, s);  // as K10's path M: no workspace, never split, the k-ascending chain
    if (rc) return rc;
    hipLaunchKernelGGL(rank_count_rows_kernel, dim3((unsigned)n_q), dim3(kBlock), 0, s, n_items, scores, st, tt, out_rank, out_score);
    hipLaunchKernelGGL(rank_exclusions_kernel, dim3((unsigned)n_q), dim3(kBlock), 0, s, a, excl_ptr, excl_idx, bitmap, words,
                       (const float*)scores, out_n_excluded);
    return mi_launch_status();
}

}  // extern "C"
