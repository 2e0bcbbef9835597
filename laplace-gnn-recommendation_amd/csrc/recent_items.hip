// N5 recent-items recommender (include/laplace_hip.h, additive to ABI 14): the three kernels between "a user's row" and
// "K items" when the user is represented by their last n_recent distinct items instead of the latest one alone.
//   mi_recent_items        one wavefront per user: lane p holds position p of the 64-entry window (p = 0 the last entry), a lane
//                          drops out when a more recent lane holds its item, slots come from a ballot and a prefix popcount.
//   mi_pool_recent_f32     pool = "mean": one lane per float4 of a query row, the rows of all slots loaded before the chain.
//   mi_topk_merge_max_f32  pool = "max": the per-slot top-K lists of one user packed into 64-bit keys in LDS, sorted by
//                          (id asc, score desc) so that run heads carry every item's best score, sorted again by
//                          (score desc, id asc); the first k_out leave.  pinsage_hard_neg_kernel's two sorts, on keys.
// No atomics, no global scratch, one writer per output: two calls give equal bits.  tests/recent_items_emulation.py restates
// the rule in numpy.
#include "common.hpp"

namespace {

constexpr int kWindow = 64;          // entries of a row that are looked at: one wavefront's lanes
constexpr int kRecentMax = MI_RECENT_MAX_SLOTS;
constexpr int kBlock = 256;
constexpr int kMergeMax = 4096;      // n_lists * k_in limit: uint64[4096] of LDS

static_assert(kWindow == MI_WAVE, "one lane per window position");

// ---- history ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void recent_items_kernel(int64_t n_users, const int32_t* __restrict__ ui_ptr,
                                                              const int32_t* __restrict__ ui_idx, int n_recent,
                                                              int64_t* __restrict__ items, int32_t* __restrict__ n_slots) {
    const int64_t u = (int64_t)blockIdx.x * (kBlock / MI_WAVE) + (threadIdx.x / MI_WAVE);
    if (u >= n_users) return;   // the whole wavefront leaves: the ballot below sees full wavefronts only
    const int lane = mi_lane();
    const int32_t end = ui_ptr[u + 1];
    const int win = min(end - ui_ptr[u], kWindow);
    const bool live = lane < win;
    const int32_t item = live ? ui_idx[end - 1 - lane] : -1;
    bool kept = live;
    for (int p = 0; p < win; ++p) {   // win is the same for every lane
        const int32_t other = __shfl(item, p, MI_WAVE);
        if (p < lane && other == item) kept = false;
    }
    const unsigned long long mask = __ballot(kept);
    const int slot = __popcll(mask & ((1ull << lane) - 1ull));
    const int ns = min(__popcll(mask), n_recent);
    const int32_t first = __shfl(item, 0, MI_WAVE);
    if (kept && slot < ns) items[(int64_t)slot * n_users + u] = (int64_t)item;
    if (lane >= ns && lane < n_recent) items[(int64_t)lane * n_users + u] = (int64_t)(win > 0 ? first : 0);
    if (lane == 0) n_slots[u] = ns;
}

// ---- pool = "mean" ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void pool_chain1(float& acc, float w, float h) {
#pragma clang fp contract(off)
    const float p = w * h;
    acc = acc + p;
}

__device__ __forceinline__ float pool_div1(float acc, float W) {
#pragma clang fp contract(off)
    return acc / W;
}

__global__ __launch_bounds__(kBlock) void pool_recent_kernel(int64_t n_users, int n_recent, int d4,
                                                             const int64_t* __restrict__ items,
                                                             const int32_t* __restrict__ n_slots, const float* __restrict__ w,
                                                             const float4* __restrict__ table, int64_t ld4,
                                                             float4* __restrict__ q, int64_t ldq4) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_users * d4) return;
    const int64_t u = i / d4;
    const int e = (int)(i - u * d4);
    const int ns = max(1, min(n_slots[u], n_recent));
    float4 x[kRecentMax];
#pragma unroll
    for (int r = 0; r < kRecentMax; ++r) {   // every slot's row load is issued before the first is used
        x[r] = mi_f4_zero();
        if (r < ns) x[r] = table[items[(int64_t)r * n_users + u] * ld4 + e];
    }
    float4 acc = mi_f4_zero();
    float W = 0.f;
#pragma unroll
    for (int r = 0; r < kRecentMax; ++r) {
        if (r < ns) {   // r < ns <= n_recent: w[r] is inside the table, and the same address for every lane
            const float wr = w[r];
            pool_chain1(acc.x, wr, x[r].x);
            pool_chain1(acc.y, wr, x[r].y);
            pool_chain1(acc.z, wr, x[r].z);
            pool_chain1(acc.w, wr, x[r].w);
            W = W + wr;
        }
    }
    q[u * ldq4 + e] = make_float4(pool_div1(acc.x, W), pool_div1(acc.y, W), pool_div1(acc.z, W), pool_div1(acc.w, W));
}

// ---- pool = "max" -------------------------------------------------------------------------------------------------------
// float -> uint32 whose unsigned order is the float order (-inf lowest, +inf highest), and back
__device__ __forceinline__ uint32_t ord_of(float f) {
    const uint32_t b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float float_of(uint32_t o) {
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o);
}

__device__ __forceinline__ float merge_score(float w, float s) {
#pragma clang fp contract(off)
    const float p = w * s;
    return p + 0.0f;   // -0 -> +0: one item never ranks by the sign of a zero
}

constexpr uint64_t kNoEntry = ~0ull;   // sorts last; no entry packs to it (ids are below 2^31)

// Ascending bitonic sort of a[0 .. P) by T threads: thread t of a step owns the pair (i, i | j), so all P / 2 compare-exchanges
// of a step are busy lanes.  For j >= 32 the 32 lanes of a half-wavefront read 32 consecutive keys (256 B: every bank once);
// below that the lanes of a half spread over 64 keys and each 8-byte read is 2-way conflicted, which is what a key-per-lane
// layout of this network costs without moving the keys into registers.
template <int P, int T>
__device__ __forceinline__ void merge_bitonic(uint64_t* a) {
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < P / 2; t += T) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int x = i | j;
                const uint64_t u = a[i], v = a[x];
                if ((u > v) == ((i & k) == 0)) { a[i] = v; a[x] = u; }
            }
            __syncthreads();
        }
}

template <int P, int T>
__global__ __launch_bounds__(T) void topk_merge_max_kernel(int n_lists, int k_in, int k_out, int64_t n_q,
                                                           const int64_t* __restrict__ ids, const float* __restrict__ scores,
                                                           const int32_t* __restrict__ n_slots, const float* __restrict__ w,
                                                           int64_t* __restrict__ out_ids, float* __restrict__ out_scores) {
    __shared__ uint64_t a[P];
    const int64_t q = blockIdx.x;
    const int tid = threadIdx.x;
    const int ns = max(0, min(n_slots[q], n_lists));
    const int E = n_lists * k_in;
    // (id asc, score desc): id << 32 | ~ord(score)
    for (int e = tid; e < P; e += T) {
        uint64_t key = kNoEntry;
        if (e < E) {
            const int l = e / k_in, j = e - l * k_in;
            if (l < ns) {
                const int64_t at = ((int64_t)l * n_q + q) * k_in + j;
                const int64_t id = ids[at];
                if (id >= 0) key = ((uint64_t)id << 32) | (uint64_t)(~ord_of(merge_score(w[l], scores[at])));
            }
        }
        a[e] = key;
    }
    __syncthreads();
    merge_bitonic<P, T>(a);
    // run heads carry the item's best score; (score desc, id asc): ~ord(score) << 32 | id
    uint64_t mine[(P + T - 1) / T];
#pragma unroll
    for (int c = 0; c < (P + T - 1) / T; ++c) {
        const int e = tid + c * T;
        uint64_t key = kNoEntry;
        if (e < P) {
            const uint64_t cur = a[e];
            if (cur != kNoEntry && (e == 0 || (a[e - 1] >> 32) != (cur >> 32))) key = (cur << 32) | (cur >> 32);
        }
        mine[c] = key;
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < (P + T - 1) / T; ++c) {
        const int e = tid + c * T;
        if (e < P) a[e] = mine[c];
    }
    __syncthreads();
    merge_bitonic<P, T>(a);
    for (int o = tid; o < k_out; o += T) {   // k_out <= k_in <= P
        const uint64_t key = a[o];
        const bool none = key == kNoEntry;
        out_ids[q * k_out + o] = none ? (int64_t)-1 : (int64_t)(key & 0xFFFFFFFFull);
        if (out_scores) out_scores[q * k_out + o] = none ? -INFINITY : float_of(~(uint32_t)(key >> 32));
    }
}

template <int P>
void merge_launch(int64_t n_q, int n_lists, int k_in, int k_out, const int64_t* ids, const float* scores, const int32_t* n_slots,
                  const float* w, int64_t* out_ids, float* out_scores, hipStream_t s) {
    constexpr int T = P / 2 < MI_WAVE ? MI_WAVE : (P / 2 > 1024 ? 1024 : P / 2);
    hipLaunchKernelGGL((topk_merge_max_kernel<P, T>), dim3((unsigned)n_q), dim3(T), 0, s, n_lists, k_in, k_out, n_q, ids, scores,
                       n_slots, w, out_ids, out_scores);
}

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

extern "C" {

int mi_recent_items(int64_t n_users, const int32_t* ui_ptr, const int32_t* ui_idx, int32_t n_recent, int64_t* items_out,
                    int32_t* n_slots_out, mi_stream_t stream) {
    MI_CHECK_ARG(n_recent >= 1 && n_users >= 0);
    if (n_recent > kRecentMax) return MI_ERR_UNSUPPORTED;
    if (n_users >= ((int64_t)1 << 31)) return MI_ERR_TOO_LARGE;
    if (n_users == 0) return 0;
    MI_CHECK_ARG(ui_ptr && ui_idx && items_out && n_slots_out);
    MI_CHECK_ARG(aligned(ui_ptr, 4) && aligned(ui_idx, 4) && aligned(items_out, 8) && aligned(n_slots_out, 4));
    // ---- nothing has been enqueued up to here ----
    hipLaunchKernelGGL(recent_items_kernel, dim3((unsigned)mi_ceil_div(n_users, kBlock / MI_WAVE)), dim3(kBlock), 0,
                       (hipStream_t)stream, n_users, ui_ptr, ui_idx, (int)n_recent, items_out, n_slots_out);
    return mi_launch_status();
}

int mi_pool_recent_f32(int64_t n_users, int32_t n_recent, int64_t d, const int64_t* items, const int32_t* n_slots, const float* w,
                       const float* table, int64_t ld, float* q_out, int64_t ldq, mi_stream_t stream) {
    MI_CHECK_ARG(n_recent >= 1 && n_users >= 0 && d >= 1);
    if (n_recent > kRecentMax || d % 4 != 0) return MI_ERR_UNSUPPORTED;
    if (n_users >= ((int64_t)1 << 31) || d >= ((int64_t)1 << 20)) return MI_ERR_TOO_LARGE;
    if (n_users == 0) return 0;
    MI_CHECK_ARG(items && n_slots && w && table && q_out);
    MI_CHECK_ARG(aligned(items, 8) && aligned(n_slots, 4) && aligned(w, 4) && mi_aligned16(table) && mi_aligned16(q_out));
    MI_CHECK_ARG(ld >= d && ld % 4 == 0 && ldq >= d && ldq % 4 == 0);
    const int64_t d4 = d / 4;
    if (n_users * d4 >= ((int64_t)INT32_MAX) * kBlock) return MI_ERR_TOO_LARGE;
    // ---- nothing has been enqueued up to here ----
    hipLaunchKernelGGL(pool_recent_kernel, dim3((unsigned)mi_ceil_div(n_users * d4, kBlock)), dim3(kBlock), 0, (hipStream_t)stream,
                       n_users, (int)n_recent, (int)d4, items, n_slots, w, reinterpret_cast<const float4*>(table), ld / 4,
                       reinterpret_cast<float4*>(q_out), ldq / 4);
    return mi_launch_status();
}

int mi_topk_merge_max_f32(int64_t n_q, int32_t n_lists, int32_t k_in, int32_t k_out, const int64_t* ids, const float* scores,
                          const int32_t* n_slots, const float* w, int64_t* out_ids, float* out_scores, mi_stream_t stream) {
    MI_CHECK_ARG(n_q >= 0 && n_lists >= 1 && k_in >= 1 && k_out >= 1 && k_out <= k_in);
    if ((int64_t)n_lists * k_in > kMergeMax) return MI_ERR_UNSUPPORTED;
    if (n_q >= ((int64_t)1 << 31)) return MI_ERR_TOO_LARGE;
    if (n_q == 0) return 0;
    MI_CHECK_ARG(ids && scores && n_slots && w && out_ids);
    MI_CHECK_ARG(aligned(ids, 8) && aligned(scores, 4) && aligned(n_slots, 4) && aligned(w, 4) && aligned(out_ids, 8) &&
                 aligned(out_scores, 4));
    // ---- nothing has been enqueued up to here ----
    const int E = n_lists * k_in;
    hipStream_t s = (hipStream_t)stream;
#define MI_MERGE_CASE(P) \
    if (E <= P) { merge_launch<P>(n_q, n_lists, k_in, k_out, ids, scores, n_slots, w, out_ids, out_scores, s); return mi_launch_status(); }
    MI_MERGE_CASE(64)
    MI_MERGE_CASE(128)
    MI_MERGE_CASE(256)
    MI_MERGE_CASE(512)
    MI_MERGE_CASE(1024)
    MI_MERGE_CASE(2048)
    MI_MERGE_CASE(4096)
#undef MI_MERGE_CASE
    return MI_ERR_UNSUPPORTED;
}

}  // extern "C"
