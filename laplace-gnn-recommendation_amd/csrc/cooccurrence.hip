// N3b: scored item co-occurrence candidates (no reference counterpart: the reference's fourth matcher keeps the first k
// entries of the user -> item -> user -> item walk and never counts them; this is the scored form of that walk).
//   mi_cooc_items_topt   stage 1: per item i the T best j by c(i, j) = (A^T A)[i, j] (or its cosine), i != j
//   mi_match_cooc_i32    stage 2: per query user the k best j by the sum of the neighbour scores of the items the user holds
//
// Stage 1, one workgroup per item row, heaviest rows first (rows bucketed by log2 of their degree; the order inside a
// bucket only decides when a row runs, never what it computes).  The row's two-hop expansion is walked once per BAND of
// item ids: dense uint32 counters over the band live in LDS and are bumped with integer LDS atomics (integer adds commute:
// exact and reproducible).  After the walk the band's candidates and the running top-T of the earlier bands go through an
// exact radix select on 64-bit keys (score bits or count | ~id: all distinct, so "the T largest" is one set whatever the
// order the atomics arrived in), and the survivors become the running top-T.  The last band ranks the <= 64 survivors.
//
// Stage 2, one workgroup per query user: the |L_u| * T (id, term) pairs — and, with exclude_seen, one marker per entry
// of the user's whole list — are sorted by (id, term index) with a bitonic network, equal ids are summed by the first
// entry of their run IN TERM ORDER (a fixed order: the float sums are reproducible), and a second sort by
// (sum descending, id ascending) brings the k best to the front.  Users whose pairs fit 4 096 slots are sorted in LDS;
// the others are queued and sorted by the same code in a slab of the workspace — exact, no truncation.
#include "common.hpp"

namespace {

// ------------------------------------------------------------------------------------------------------------------
// stage 1
// ------------------------------------------------------------------------------------------------------------------
constexpr int kS1Block = 1024;
constexpr int kMaxT = 64;
constexpr int kBandMax = 36864;          // counters per band: 144 KiB of the CU's 160 KiB (105 542 items = 3 bands)
constexpr int kHistBins = 2048;          // 11-bit digits
constexpr int kBuckets = 32;

struct S1Shared {                         // the fixed part of the LDS image; the band's counters follow it
    uint32_t hist[kHistBins];
    uint32_t super[kHistBins / MI_WAVE];
    uint64_t run_key[kMaxT];
    uint64_t new_key[kMaxT];
    uint32_t run_cnt[kMaxT];
    uint32_t new_cnt[kMaxT];
    uint64_t prefix;
    uint32_t need, n_run, n_new, total;
};

__host__ __device__ inline int s1_bucket(int32_t d) {   // 0 = heaviest
    int lg = 0;
    while (lg < 31 && (d >> (lg + 1)) != 0) ++lg;        // floor(log2(d)), d >= 1
    return d <= 0 ? kBuckets - 1 : 30 - lg;
}

__global__ void cooc_bucket_count_kernel(int32_t n_items, const int32_t* __restrict__ aptr, int32_t* __restrict__ counts) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_items) atomicAdd(&counts[s1_bucket(aptr[i + 1] - aptr[i])], 1);
}

__global__ void cooc_bucket_place_kernel(int32_t n_items, const int32_t* __restrict__ aptr, const int32_t* __restrict__ counts,
                                         int32_t* __restrict__ cursor, int32_t* __restrict__ order) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_items) return;
    const int b = s1_bucket(aptr[i + 1] - aptr[i]);
    int32_t start = 0;
    for (int x = 0; x < b; ++x) start += counts[x];
    order[start + atomicAdd(&cursor[b], 1)] = (int32_t)i;
}

// the lane holding the highest v-slot whose suffix sum (that slot and all above it) reaches `need`; `above` = the sum
// strictly above it.  Whole wave, v = 0 in unused lanes.
__device__ __forceinline__ int s1_suffix_pick(uint32_t v, uint32_t need, uint32_t& above) {
    const int lane = mi_lane();
    uint32_t s = v;
#pragma unroll
    for (int off = 1; off < MI_WAVE; off <<= 1) {
        const uint32_t o = __shfl_down(s, off, MI_WAVE);
        if (lane + off < MI_WAVE) s += o;
    }
    const uint64_t m = __ballot(s >= need);
    const int pick = m ? 63 - __clzll((long long)m) : 0;
    above = __shfl(s, pick, MI_WAVE) - __shfl(v, pick, MI_WAVE);
    return pick;
}

template <bool kCosine>
__device__ __forceinline__ uint64_t s1_key(uint32_t c, int32_t j, int32_t d_i, const int32_t* __restrict__ aptr) {
    uint32_t hi;
    if (kCosine) {  // c / sqrt(d_i * d_j), every rounding explicit
        const int32_t d_j = aptr[j + 1] - aptr[j];
        hi = __float_as_uint(__fdiv_rn((float)c, __fsqrt_rn(__fmul_rn((float)d_i, (float)d_j))));
    } else {
        hi = c;
    }
    return ((uint64_t)hi << 32) | (uint32_t)(0xFFFFFFFFu - (uint32_t)j);
}

template <bool kCosine>
__global__ __launch_bounds__(kS1Block) void cooc_items_kernel(int32_t n_items, int32_t band, int32_t T,
                                                              const int32_t* __restrict__ order,
                                                              const int32_t* __restrict__ uptr, const int32_t* __restrict__ uidx,
                                                              const int32_t* __restrict__ aptr, const int32_t* __restrict__ aidx,
                                                              int32_t* __restrict__ nbr_id, int32_t* __restrict__ nbr_count,
                                                              float* __restrict__ nbr_score) {
    extern __shared__ __align__(16) unsigned char s1_lds[];
    S1Shared& sh = *reinterpret_cast<S1Shared*>(s1_lds);
    uint32_t* cnt = reinterpret_cast<uint32_t*>(s1_lds + sizeof(S1Shared));
    const int tid = threadIdx.x, lane = mi_lane(), wave = tid / MI_WAVE;
    constexpr int kWaves = kS1Block / MI_WAVE;
    const int32_t i = order[blockIdx.x];
    const int32_t a0 = aptr[i], a1 = aptr[i + 1], d_i = a1 - a0;
    int32_t* o_id = nbr_id + (int64_t)i * T;
    int32_t* o_cnt = nbr_count + (int64_t)i * T;
    float* o_sc = nbr_score + (int64_t)i * T;
    if (d_i == 0) {  // nobody bought it: no neighbours
        for (int x = tid; x < T; x += kS1Block) { o_id[x] = -1; o_cnt[x] = 0; o_sc[x] = 0.f; }
        return;
    }
    if (tid == 0) sh.n_run = 0;

    for (int32_t b0 = 0; b0 < n_items; b0 += band) {
        const int32_t bw = min(band, n_items - b0);
        for (int x = tid; x < bw; x += kS1Block) cnt[x] = 0;
        if (tid == 0) { sh.total = 0; sh.n_new = 0; }
        __syncthreads();
        // the walk i -> u -> j: 16 lanes per user of the row, every position of both lists counts
        for (int32_t p = a0 + tid / 16; p < a1; p += kS1Block / 16) {
            const int32_t u = aidx[p];
            const int32_t q1 = uptr[u + 1];
            for (int32_t q = uptr[u] + (tid & 15); q < q1; q += 16) {
                const int32_t j = uidx[q];
                const uint32_t rel = (uint32_t)(j - b0);
                if (j != i && rel < (uint32_t)bw) atomicAdd(&cnt[rel], 1u);
            }
        }
        __syncthreads();
        const uint32_t n_run = sh.n_run;
        // candidates = the band's non-zero counters + the running top-T
        {
            uint32_t mine = 0;
            for (int x = tid; x < bw; x += kS1Block) mine += cnt[x] != 0;
            for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off, MI_WAVE);
            if (lane == 0 && mine) atomicAdd(&sh.total, mine);
        }
        __syncthreads();
        const uint32_t total = sh.total + n_run;
        uint64_t thr = 0;  // keep every candidate with key >= thr
        if (total > (uint32_t)T) {
            // exact radix select of the T-th largest key: digits of 11, 11, 10 bits over each half of the key
            if (tid == 0) { sh.prefix = 0; sh.need = (uint32_t)T; }
            for (int pass = 0; pass < 6; ++pass) {
                const int width = (pass % 3 == 2) ? 10 : 11;
                const int shift = pass == 0 ? 53 : pass == 1 ? 42 : pass == 2 ? 32 : pass == 3 ? 21 : pass == 4 ? 10 : 0;
                for (int x = tid; x < kHistBins; x += kS1Block) sh.hist[x] = 0;
                __syncthreads();
                const uint64_t prefix = sh.prefix;
                const uint32_t need = sh.need;
                auto vote = [&](uint64_t key) {
                    if (pass == 0 || (key >> (shift + width)) == prefix)
                        atomicAdd(&sh.hist[(uint32_t)(key >> shift) & ((1u << width) - 1u)], 1u);
                };
                for (int x = tid; x < bw; x += kS1Block) {
                    const uint32_t c = cnt[x];
                    if (c) vote(s1_key<kCosine>(c, b0 + x, d_i, aptr));
                }
                if ((uint32_t)tid < n_run) vote(sh.run_key[tid]);
                __syncthreads();
                for (int sb = wave; sb < kHistBins / MI_WAVE; sb += kWaves) {
                    uint32_t v = sh.hist[sb * MI_WAVE + lane];
                    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, MI_WAVE);
                    if (lane == 0) sh.super[sb] = v;
                }
                __syncthreads();
                if (wave == 0) {
                    uint32_t above_sb, above_d;
                    const int sb = s1_suffix_pick(lane < kHistBins / MI_WAVE ? sh.super[lane] : 0u, need, above_sb);
                    const int dg = s1_suffix_pick(sh.hist[sb * MI_WAVE + lane], need - above_sb, above_d);
                    if (lane == 0) {
                        sh.prefix = (prefix << width) | (uint64_t)(sb * MI_WAVE + dg);
                        sh.need = need - above_sb - above_d;
                    }
                }
                __syncthreads();
            }
            thr = sh.prefix;
        }
        // the survivors (at most T: the keys are distinct) become the running top-T
        auto keep = [&](uint64_t key, uint32_t c) {
            if (key >= thr) {
                const uint32_t slot = atomicAdd(&sh.n_new, 1u);
                if (slot < (uint32_t)kMaxT) { sh.new_key[slot] = key; sh.new_cnt[slot] = c; }
            }
        };
        for (int x = tid; x < bw; x += kS1Block) {
            const uint32_t c = cnt[x];
            if (c) keep(s1_key<kCosine>(c, b0 + x, d_i, aptr), c);
        }
        if ((uint32_t)tid < n_run) keep(sh.run_key[tid], sh.run_cnt[tid]);
        __syncthreads();
        const uint32_t n_new = min(sh.n_new, (uint32_t)T);
        if ((uint32_t)tid < n_new) { sh.run_key[tid] = sh.new_key[tid]; sh.run_cnt[tid] = sh.new_cnt[tid]; }
        if (tid == 0) sh.n_run = n_new;
        __syncthreads();
    }
    // rank the survivors: (score descending, id ascending) = key descending
    const uint32_t n_run = sh.n_run;
    if ((uint32_t)tid < n_run) {
        const uint64_t key = sh.run_key[tid];
        uint32_t rank = 0;
        for (uint32_t x = 0; x < n_run; ++x) rank += sh.run_key[x] > key;
        const uint32_t c = sh.run_cnt[tid];
        o_id[rank] = (int32_t)(0xFFFFFFFFu - (uint32_t)key);
        o_cnt[rank] = (int32_t)c;
        o_sc[rank] = kCosine ? __uint_as_float((uint32_t)(key >> 32)) : (float)c;
    }
    for (int x = (int)n_run + tid; x < T; x += kS1Block) { o_id[x] = -1; o_cnt[x] = 0; o_sc[x] = 0.f; }
}

inline int32_t s1_band(int64_t n_items) { return (int32_t)(n_items < kBandMax ? (n_items > 0 ? n_items : 1) : kBandMax); }

// ------------------------------------------------------------------------------------------------------------------
// stage 2
// ------------------------------------------------------------------------------------------------------------------
constexpr int kS2Block = 256;
constexpr int kS2BigBlock = 1024;
constexpr int kS2LdsSlots = 4096;        // 32 KiB of keys per workgroup
constexpr int kS2MaxSlabs = 256;
constexpr uint32_t kMarker = 0xFFFFFFFFu;  // low word of a "the user holds this item" entry: sorts last among its id
constexpr uint32_t kHead = 0x80000000u;

struct S2Args {
    const int64_t* q_users;
    const int32_t* uptr;
    const int32_t* uidx;
    const int32_t* nbr_id;
    const float* nbr_score;
    int32_t T, k, n_recent, exclude_seen;
    int32_t* out;
    float* out_score;
    int32_t* out_count;
};

__host__ __device__ inline int64_t s2_pow2(int64_t n) {
    int64_t p = 64;
    while (p < n) p <<= 1;
    return p;
}

// in-place bitonic sort of buf[0, N), N a power of two, by the whole workgroup; buf in LDS or in global memory
__device__ __forceinline__ void s2_sort(uint64_t* buf, int N, bool descending) {
    for (int size = 2; size <= N; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int x = threadIdx.x; x < (N >> 1); x += blockDim.x) {
                const int lo = 2 * x - (x & (stride - 1));
                const int hi = lo + stride;
                const uint64_t a = buf[lo], b = buf[hi];
                const bool up = ((lo & size) == 0) != descending;
                if ((a > b) == up) { buf[lo] = b; buf[hi] = a; }
            }
            __syncthreads();
        }
    }
}

__device__ __forceinline__ void s2_write_empty(const S2Args& a, int64_t q, int32_t count) {
    for (int x = threadIdx.x; x < a.k; x += blockDim.x) {
        a.out[q * a.k + x] = -1;
        if (a.out_score) a.out_score[q * a.k + x] = 0.f;
    }
    if (a.out_count && threadIdx.x == 0) a.out_count[q] = count;
}

__device__ __forceinline__ void s2_user_shape(const S2Args& a, int64_t q, int32_t& l0, int32_t& l1, int32_t& first, int64_t& n_terms,
                                              int64_t& n_all) {
    const int64_t u = a.q_users ? a.q_users[q] : q;
    l0 = a.uptr[u];
    l1 = a.uptr[u + 1];
    first = (a.n_recent > 0 && l1 - l0 > a.n_recent) ? l1 - a.n_recent : l0;   // list order is transaction order
    n_terms = (int64_t)(l1 - first) * a.T;
    n_all = n_terms + (a.exclude_seen ? (l1 - l0) : 0);
}

__device__ __forceinline__ void s2_match_one(const S2Args& a, int64_t q, uint64_t* buf, int N, int32_t l0, int32_t l1, int32_t first,
                                             int64_t n_terms, int64_t n_all) {
    const int T = a.T;
    // 1. (id << 32 | term index) per neighbour entry, (id << 32 | marker) per held item, all-ones pads
    for (int x = threadIdx.x; x < N; x += blockDim.x) {
        uint64_t key = ~0ull;
        if (x < n_terms) {
            const int32_t id = a.nbr_id[(int64_t)a.uidx[first + x / T] * T + x % T];
            if (id >= 0) key = ((uint64_t)(uint32_t)id << 32) | (uint32_t)x;
        } else if (x < n_all) {
            key = ((uint64_t)(uint32_t)a.uidx[l0 + (x - n_terms)] << 32) | kMarker;
        }
        buf[x] = key;
    }
    __syncthreads();
    s2_sort(buf, N, false);
    // 2. flag the first entry of every run of one id (bit 63; ids are below 2^31, pads carry it already) ...
    for (int x0 = 0; x0 < N; x0 += blockDim.x) {
        const int x = x0 + threadIdx.x;
        bool head = false;
        if (x < N) {
            const uint32_t id = (uint32_t)(buf[x] >> 32);
            // the entry before may or may not carry its flag yet (the previous round of this loop writes it): compare ids only
            head = id != 0xFFFFFFFFu && (x == 0 || ((uint32_t)(buf[x - 1] >> 32) & ~kHead) != id);
        }
        __syncthreads();
        if (head) buf[x] |= (uint64_t)kHead << 32;
    }
    __syncthreads();
    // ... which sums its run in term order and leaves the sum in its own low word (0 = dropped)
    for (int x = threadIdx.x; x < N; x += blockDim.x) {
        const uint64_t key = buf[x];
        const uint32_t hi = (uint32_t)(key >> 32);
        if (hi == 0xFFFFFFFFu || !(hi & kHead)) continue;
        float r = 0.f;
        bool seen = false;
        uint32_t low = (uint32_t)key;
        for (int y = x;;) {
            if (low == kMarker) seen = true;
            else r = __fadd_rn(r, a.nbr_score[(int64_t)a.uidx[first + low / T] * T + low % T]);
            if (++y >= N) break;
            const uint64_t nk = buf[y];
            if ((uint32_t)(nk >> 32) & kHead) break;
            low = (uint32_t)nk;
        }
        reinterpret_cast<uint32_t*>(buf + x)[0] = (seen || !(r > 0.f)) ? 0u : __float_as_uint(r);   // little endian: the low word
    }
    __syncthreads();
    // 3. (sum bits << 32 | ~id) for the kept heads, 0 for everything else; the k largest first
    for (int x = threadIdx.x; x < N; x += blockDim.x) {
        const uint64_t key = buf[x];
        const uint32_t hi = (uint32_t)(key >> 32), low = (uint32_t)key;
        buf[x] = (hi != 0xFFFFFFFFu && (hi & kHead) && low) ? ((uint64_t)low << 32) | (0xFFFFFFFFu - (hi & ~kHead)) : 0ull;
    }
    __syncthreads();
    s2_sort(buf, N, true);
    const int lim = min(a.k, N);
    for (int x = threadIdx.x; x < a.k; x += blockDim.x) {
        const uint64_t key = x < lim ? buf[x] : 0ull;
        a.out[q * a.k + x] = key ? (int32_t)(0xFFFFFFFFu - (uint32_t)key) : -1;
        if (a.out_score) a.out_score[q * a.k + x] = key ? __uint_as_float((uint32_t)(key >> 32)) : 0.f;
        if (a.out_count) {
            if (key && (x + 1 == lim || buf[x + 1] == 0ull)) a.out_count[q] = x + 1;
            if (x == 0 && !key) a.out_count[q] = 0;
        }
    }
}

__global__ __launch_bounds__(kS2Block) void match_cooc_kernel(int64_t n_q, S2Args a, int32_t* __restrict__ big_n,
                                                              int32_t* __restrict__ big_list, int64_t slab_slots) {
    __shared__ uint64_t keys[kS2LdsSlots];
    const int64_t q = blockIdx.x;
    int32_t l0, l1, first;
    int64_t n_terms, n_all;
    s2_user_shape(a, q, l0, l1, first, n_terms, n_all);
    if (n_terms == 0) { s2_write_empty(a, q, 0); return; }
    if (n_all > kS2LdsSlots) {  // sorted in a slab of the workspace by match_cooc_big_kernel
        if (s2_pow2(n_all) > slab_slots) { s2_write_empty(a, q, -1); return; }   // longer than the caller's max_list_len: refused, not truncated
        if (threadIdx.x == 0) big_list[atomicAdd(big_n, 1)] = (int32_t)q;
        return;
    }
    s2_match_one(a, q, keys, (int)s2_pow2(n_all), l0, l1, first, n_terms, n_all);
}

__global__ __launch_bounds__(kS2BigBlock) void match_cooc_big_kernel(S2Args a, const int32_t* __restrict__ big_n,
                                                                     const int32_t* __restrict__ big_list, uint64_t* __restrict__ slabs,
                                                                     int64_t slab_slots) {
    uint64_t* buf = slabs + (int64_t)blockIdx.x * slab_slots;
    const int32_t n = *big_n;
    for (int32_t e = blockIdx.x; e < n; e += gridDim.x) {
        const int64_t q = big_list[e];
        int32_t l0, l1, first;
        int64_t n_terms, n_all;
        s2_user_shape(a, q, l0, l1, first, n_terms, n_all);
        const int64_t N = s2_pow2(n_all);
        s2_match_one(a, q, buf, (int)N, l0, l1, first, n_terms, n_all);
        __syncthreads();
    }
}

inline int64_t s2_slab_slots(int64_t max_list_len, int32_t T) {
    const int64_t worst = max_list_len * ((int64_t)T + 1);
    return worst > kS2LdsSlots ? s2_pow2(worst) : 0;
}

inline int64_t s2_n_slabs(int64_t n_queries) { return n_queries < kS2MaxSlabs ? n_queries : kS2MaxSlabs; }

}  // namespace

extern "C" size_t mi_cooc_items_workspace_bytes(int64_t n_items, int64_t nnz, int32_t T) {
    if (n_items < 0 || n_items >= INT32_MAX || nnz < 0 || nnz >= ((int64_t)1 << 31) || T < 1 || T > kMaxT) return 0;
    return 256 + mi_align_up((size_t)(n_items > 0 ? n_items : 1) * sizeof(int32_t), 256);
}

extern "C" int mi_cooc_items_topt(int64_t n_users, int64_t n_items, int64_t nnz, const int32_t* users_ptr, const int32_t* users_idx,
                                  const int32_t* articles_ptr, const int32_t* articles_idx, int32_t T, int32_t weighting,
                                  int32_t* nbr_id, int32_t* nbr_count, float* nbr_score, void* ws, size_t ws_bytes,
                                  mi_stream_t stream) {
    MI_CHECK_ARG(n_users >= 0 && n_users < INT32_MAX && n_items >= 0 && n_items < INT32_MAX);
    MI_CHECK_ARG(nnz >= 0 && nnz < ((int64_t)1 << 31));
    MI_CHECK_ARG(T >= 1 && T <= kMaxT && (weighting == MI_COOC_COUNT || weighting == MI_COOC_COSINE));
    if (n_items == 0) return 0;
    MI_CHECK_ARG(users_ptr && articles_ptr && nbr_id && nbr_count && nbr_score && ws);
    MI_CHECK_ARG(nnz == 0 || (users_idx && articles_idx));
    if (ws_bytes < mi_cooc_items_workspace_bytes(n_items, nnz, T)) return MI_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    MiArena ar(ws, ws_bytes);
    int32_t* counters = ar.take<int32_t>(2 * kBuckets);   // [bucket sizes | cursors]
    int32_t* order = ar.take<int32_t>((size_t)n_items);
    if (!counters || !order) return MI_ERR_WORKSPACE;
    MI_HIP(hipMemsetAsync(counters, 0, 2 * kBuckets * sizeof(int32_t), s));
    const unsigned grid = (unsigned)mi_ceil_div(n_items, 256);
    hipLaunchKernelGGL(cooc_bucket_count_kernel, dim3(grid), dim3(256), 0, s, (int32_t)n_items, articles_ptr, counters);
    hipLaunchKernelGGL(cooc_bucket_place_kernel, dim3(grid), dim3(256), 0, s, (int32_t)n_items, articles_ptr, counters,
                       counters + kBuckets, order);
    const int32_t band = s1_band(n_items);
    const size_t lds = sizeof(S1Shared) + (size_t)band * sizeof(uint32_t);
    auto kern = weighting == MI_COOC_COSINE ? cooc_items_kernel<true> : cooc_items_kernel<false>;
    if (lds > 65536 &&
        hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return MI_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(kern, dim3((unsigned)n_items), dim3(kS1Block), lds, s, (int32_t)n_items, band, T, order, users_ptr, users_idx,
                       articles_ptr, articles_idx, nbr_id, nbr_count, nbr_score);
    return mi_launch_status();
}

extern "C" size_t mi_match_cooc_workspace_bytes(int64_t n_queries, int64_t max_list_len, int32_t T) {
    if (n_queries < 0 || n_queries >= INT32_MAX || max_list_len < 0 || max_list_len >= ((int64_t)1 << 31) || T < 1 || T > kMaxT)
        return 0;
    return 256 + mi_align_up((size_t)(n_queries > 0 ? n_queries : 1) * sizeof(int32_t), 256) +
           (size_t)s2_n_slabs(n_queries) * (size_t)s2_slab_slots(max_list_len, T) * sizeof(uint64_t);
}

extern "C" int mi_match_cooc_i32(int64_t n_queries, const int64_t* query_users, const int32_t* users_ptr, const int32_t* users_idx,
                                 int64_t max_list_len, int32_t T, const int32_t* nbr_id, const float* nbr_score, int32_t k,
                                 int32_t n_recent, int32_t exclude_seen, int32_t* out, float* out_score, int32_t* out_count,
                                 void* ws, size_t ws_bytes, mi_stream_t stream) {
    MI_CHECK_ARG(n_queries >= 0 && n_queries < INT32_MAX && k > 0 && T >= 1 && T <= kMaxT);
    MI_CHECK_ARG(max_list_len >= 0 && max_list_len < ((int64_t)1 << 31) && s2_slab_slots(max_list_len, T) <= ((int64_t)1 << 30));
    if (n_queries == 0) return 0;
    MI_CHECK_ARG(users_ptr && users_idx && nbr_id && nbr_score && out && ws);
    if (ws_bytes < mi_match_cooc_workspace_bytes(n_queries, max_list_len, T)) return MI_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    MiArena ar(ws, ws_bytes);
    int32_t* big_n = ar.take<int32_t>(1);
    int32_t* big_list = ar.take<int32_t>((size_t)n_queries);
    const int64_t slab_slots = s2_slab_slots(max_list_len, T);
    const int64_t n_slabs = s2_n_slabs(n_queries);
    uint64_t* slabs = slab_slots ? ar.take<uint64_t>((size_t)(n_slabs * slab_slots)) : nullptr;
    if (!big_n || !big_list || (slab_slots && !slabs)) return MI_ERR_WORKSPACE;
    const S2Args a = {query_users, users_ptr, users_idx, nbr_id, nbr_score, T, k, n_recent > 0 ? n_recent : 0, exclude_seen != 0,
                      out, out_score, out_count};
    MI_HIP(hipMemsetAsync(big_n, 0, sizeof(int32_t), s));
    hipLaunchKernelGGL(match_cooc_kernel, dim3((unsigned)n_queries), dim3(kS2Block), 0, s, n_queries, a, big_n, big_list, slab_slots);
    if (slab_slots)
        hipLaunchKernelGGL(match_cooc_big_kernel, dim3((unsigned)n_slabs), dim3(kS2BigBlock), 0, s, a, big_n, big_list, slabs, slab_slots);
    return mi_launch_status();
}
