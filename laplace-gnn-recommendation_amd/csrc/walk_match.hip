// N3c random-walk matcher (include/laplace_hip.h, additive to ABI 14): Pixie-style candidates for a USER, by walking from the
// items they hold.  No table, no training: an edge counts the moment it is in the CSR.
//
// One workgroup per query user:
//   history   the first wavefront finds the user's slots as recent_items_kernel does (csrc/recent_items.hip): lane p holds
//             position p of the 64-entry window, a lane drops out when a more recent lane holds its item.
//   walks     walk w starts at slot w % R; the walks run side by side, strided over the threads (each is a chain of dependent
//             global loads, as in pinsage_hard_neg_kernel); a traversal end lands in LDS as the key (item << 4) | slot,
//             kNone (sorts last) where the walk had ended before.
//   count     a first bitonic sort makes an item's slot-runs adjacent.  The first key of an item folds the item's runs, at
//             most 16, in ascending slot order: every run's end is a binary search (run length = c[r][i]).
//   select    exclude_seen is a binary search in the row-sorted copy of the user's row; survivors become
//             (~score bits << 32) | item, a second sort orders them by (score desc, id asc), the first k leave.
// Integer counts, one thread per item's fold, no atomics, no global scratch: two calls give equal bits, and
// tests/random_walk_matcher_emulation.py restates the rule in numpy draw for draw.
#include "common.hpp"
#include "walk_law.hpp"

namespace {

enum { P_MATCH_WALK = 17 };          // purposes 11-16: csrc/pinsage.hip

constexpr int kWindow = 64;          // entries of a row that are looked at: one wavefront's lanes
constexpr int kSlotBits = 4;         // MI_RECENT_MAX_SLOTS = 16 slot numbers below the item id
constexpr int kMaxThreads = 1024;
constexpr int kKeysPerThread = MI_WALK_MATCH_MAX_VISITS / kMaxThreads;   // 4 at the limit; launches of P / 2 threads hold 2
constexpr uint64_t kNone = ~0ull;    // sorts last; no key packs to it (ids are below 2^31 - 1, a score is never 0)

static_assert(kWindow == MI_WAVE, "one lane per window position");
static_assert((1 << kSlotBits) == MI_RECENT_MAX_SLOTS, "a slot number fits the key's low bits");
static_assert(kKeysPerThread >= 2, "P / 2 threads hold two keys each");

// Ascending bitonic sort of a[0 .. P), P a power of two: thread t of a step owns the pair (i, i | j) (recent_items.hip's
// network, with the sizes known at run time only).
__device__ __forceinline__ void walk_bitonic(uint64_t* a, int P) {
    const int T = blockDim.x;
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

__device__ __forceinline__ int walk_lower_bound(const uint64_t* a, int n, uint64_t key) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// is `item` in sorted[lo .. end)?  (entries lo .. end - 1 ascending)
__device__ __forceinline__ bool row_holds(const int32_t* __restrict__ sorted, int32_t lo, int32_t end, int32_t item) {
    int32_t hi = end;
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (sorted[mid] < item) lo = mid + 1; else hi = mid;
    }
    return lo < end && sorted[lo] == item;
}

// multi_hit: acc = acc + sqrt(c), one rounding per operation; sqrtf is the correctly rounded sequence (the default
// -fhip-fp32-correctly-rounded-divide-sqrt), and 0 + x is x
__device__ __forceinline__ float boost_add_root(float acc, int c) {
#pragma clang fp contract(off)
    const float r = sqrtf((float)c);
    return acc + r;
}
__device__ __forceinline__ float boost_square(float acc) {
#pragma clang fp contract(off)
    return acc * acc;
}

struct WalkMatchArgs {
    Bip g;
    const int32_t* ui_sorted;        // the user -> item rows sorted by id (exclude_seen), null otherwise
    const int64_t* query_users;      // null: query q is user q
    int64_t n_users;
    int num_walks, walk_length, n_recent, k, boost, visits, P;
    uint32_t restart_thr;
    uint64_t seed, step;
    int32_t* out_ids;
    float* out_scores;
    int32_t* out_count;
};

__global__ __launch_bounds__(kMaxThreads) void walk_match_kernel(WalkMatchArgs a) {
    __shared__ uint64_t A[MI_WALK_MATCH_MAX_VISITS];
    __shared__ int32_t slot_item[MI_RECENT_MAX_SLOTS];
    __shared__ int n_slots;
    const int tid = threadIdx.x, T = blockDim.x;
    const int64_t q = blockIdx.x;
    const int64_t u = a.query_users ? a.query_users[q] : q;
    const bool known = u >= 0 && u < a.n_users;      // an id outside the graph has no row: no proposal, nothing is read
    const int32_t row_lo = known ? a.g.ui_ptr[u] : 0, row_hi = known ? a.g.ui_ptr[u + 1] : 0;

    if (tid < MI_WAVE) {   // the whole first wavefront: the ballot below sees a full wavefront
        const int win = min(row_hi - row_lo, kWindow);
        const bool live = tid < win;
        const int32_t item = live ? a.g.ui_idx[row_hi - 1 - tid] : -1;
        bool kept = live;
        for (int p = 0; p < win; ++p) {   // win is the same for every lane
            const int32_t other = __shfl(item, p, MI_WAVE);
            if (p < tid && other == item) kept = false;
        }
        const unsigned long long mask = __ballot(kept);
        const int slot = __popcll(mask & ((1ull << tid) - 1ull));
        const int ns = min(__popcll(mask), a.n_recent);
        if (kept && slot < ns) slot_item[slot] = item;
        if (tid == 0) n_slots = ns;
    }
    __syncthreads();
    const int R = n_slots;
    if (R == 0) {   // an empty row: no proposal (the same test for every thread of the workgroup)
        for (int o = tid; o < a.k; o += T) {
            a.out_ids[q * a.k + o] = -1;
            if (a.out_scores) a.out_scores[q * a.k + o] = 0.f;
        }
        if (a.out_count && tid == 0) a.out_count[q] = 0;
        return;
    }

    const int P = a.P, L = a.walk_length;
    for (int i = a.visits + tid; i < P; i += T) A[i] = kNone;
    for (int w = tid; w < a.num_walks; w += T) {
        const int r = w % R;
        int32_t cur = slot_item[r];
        int tr = 0;
        for (; tr < L; ++tr) {
            const MiPhilox x = pw(P_MATCH_WALK, (uint32_t)(w * L + tr), 0, (uint32_t)u, a.seed, a.step);
            if (tr > 0 && x.c[2] < a.restart_thr) break;
            cur = hop(a.g, cur, x.c[0], x.c[1]);
            if (cur == -1) break;
            A[w * L + tr] = ((uint64_t)(uint32_t)cur << kSlotBits) | (uint64_t)r;
        }
        for (; tr < L; ++tr) A[w * L + tr] = kNone;
    }
    __syncthreads();
    walk_bitonic(A, P);

    // the first key of an item folds the item's slot-runs into its score
    uint64_t mine[kKeysPerThread];
#pragma unroll
    for (int c = 0; c < kKeysPerThread; ++c) {
        const int e = tid + c * T;
        uint64_t key = kNone;
        if (e < P) {
            const uint64_t cur = A[e];
            const uint64_t item = cur >> kSlotBits;
            if (cur != kNone && (e == 0 || (A[e - 1] >> kSlotBits) != item)) {
                int pos = e, total = 0;
                float acc = 0.f;
                while (pos < P && (A[pos] >> kSlotBits) == item) {   // at most 16 runs, ascending slot
                    const int end = walk_lower_bound(A, P, A[pos] + 1);   // kNone is never a run: A[pos] + 1 does not wrap
                    const int cnt = end - pos;
                    total += cnt;
                    if (a.boost == MI_WALK_BOOST_MULTI_HIT) acc = boost_add_root(acc, cnt);
                    pos = end;
                }
                const float s = a.boost == MI_WALK_BOOST_MULTI_HIT ? boost_square(acc) : (float)total;
                if (!(a.ui_sorted && row_holds(a.ui_sorted, row_lo, row_hi, (int32_t)item)))
                    key = ((uint64_t)(~__float_as_uint(s)) << 32) | item;   // s > 0: its bits order as its value
            }
        }
        mine[c] = key;
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < kKeysPerThread; ++c) {
        const int e = tid + c * T;
        if (e < P) A[e] = mine[c];
    }
    __syncthreads();
    walk_bitonic(A, P);

    for (int o = tid; o < a.k; o += T) {
        const uint64_t key = o < P ? A[o] : kNone;
        const bool none = key == kNone;
        a.out_ids[q * a.k + o] = none ? -1 : (int32_t)(key & 0xFFFFFFFFull);
        if (a.out_scores) a.out_scores[q * a.k + o] = none ? 0.f : __uint_as_float(~(uint32_t)(key >> 32));
    }
    if (a.out_count && tid == 0) a.out_count[q] = walk_lower_bound(A, P, kNone);   // distinct eligible items, before the cut
}

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

extern "C" {

int mi_match_random_walks_i32(int64_t n_queries, const int64_t* query_users, int64_t n_users, int64_t n_items,
                              const int32_t* iu_ptr, const int32_t* iu_idx, const int32_t* ui_ptr, const int32_t* ui_idx,
                              const int32_t* ui_sorted, int32_t k, int32_t num_walks, int32_t walk_length, double restart_prob,
                              int32_t n_recent, int32_t boost, int32_t exclude_seen, uint64_t seed, uint64_t step,
                              int32_t* out_ids, float* out_scores, int32_t* out_count, mi_stream_t stream) {
    MI_CHECK_ARG(n_queries >= 0 && n_users >= 0 && n_items >= 0);
    MI_CHECK_ARG(k > 0 && num_walks > 0 && walk_length > 0);
    MI_CHECK_ARG(restart_prob >= 0.0 && restart_prob < 1.0);   // NaN fails both
    MI_CHECK_ARG(n_recent >= 1 && n_recent <= MI_RECENT_MAX_SLOTS);
    MI_CHECK_ARG(boost == MI_WALK_BOOST_SUM || boost == MI_WALK_BOOST_MULTI_HIT);
    if ((int64_t)num_walks * walk_length > MI_WALK_MATCH_MAX_VISITS) return MI_ERR_UNSUPPORTED;
    if (n_items >= (int64_t)INT32_MAX || n_users >= (int64_t)INT32_MAX || n_queries >= (int64_t)INT32_MAX) return MI_ERR_TOO_LARGE;
    if ((int64_t)n_queries * k >= ((int64_t)1 << 40)) return MI_ERR_TOO_LARGE;
    if (n_queries == 0) return 0;
    MI_CHECK_ARG(iu_ptr && iu_idx && ui_ptr && ui_idx && out_ids && (!exclude_seen || ui_sorted));
    MI_CHECK_ARG(aligned(query_users, 8) && aligned(iu_ptr, 4) && aligned(iu_idx, 4) && aligned(ui_ptr, 4) && aligned(ui_idx, 4) &&
                 aligned(ui_sorted, 4) && aligned(out_ids, 4) && aligned(out_scores, 4) && aligned(out_count, 4));
    // ---- nothing has been enqueued up to here ----
    WalkMatchArgs a;
    a.g = {iu_ptr, iu_idx, ui_ptr, ui_idx};
    a.ui_sorted = exclude_seen ? ui_sorted : nullptr;
    a.query_users = query_users;
    a.n_users = n_users;
    a.num_walks = num_walks;
    a.walk_length = walk_length;
    a.n_recent = n_recent;
    a.k = k;
    a.boost = boost;
    a.visits = num_walks * walk_length;
    int P = 2;
    while (P < a.visits) P <<= 1;
    a.P = P;
    a.restart_thr = (uint32_t)(restart_prob * 4294967296.0);
    a.seed = seed;
    a.step = step;
    a.out_ids = out_ids;
    a.out_scores = out_scores;
    a.out_count = out_count;
    // a thread per compare-exchange of a sort step, a wavefront at least (the history needs one), 1024 at most
    const int threads = P / 2 < MI_WAVE ? MI_WAVE : (P / 2 > kMaxThreads ? kMaxThreads : P / 2);
    hipLaunchKernelGGL(walk_match_kernel, dim3((unsigned)n_queries), dim3(threads), 0, (hipStream_t)stream, a);
    return mi_launch_status();
}

}  // extern "C"
