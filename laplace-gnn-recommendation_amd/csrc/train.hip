// LightGCN training-step kernels other than the propagate:
//   K9   mi_sample_bpr_batch   data/lightgcn_loader.py:95-112 (+ PyG structured_negative_sampling)
//   a7/8 mi_bpr_fwd_bwd_f32    run_pipeline_lightgcn.py:133-155, utils/metrics_lightgcn.py:9-45
//   a9   mi_adam_dense_f32     run_pipeline_lightgcn.py:157-159 (torch.optim.Adam)
// and, not in the reference (SURVEY F9 behind a flag): the ranking objectives over M negatives (mi_rank_loss_fwd_bwd_f32),
// popularity-weighted negatives (mi_sample_bpr_batch_pop) and the logQ-corrected softmax (mi_rank_loss_fwd_bwd_lq_f32).
// The reference's entries are the (MI_RANK_REFERENCE, one negative) case of the general ones and launch what those launch
// at n_neg = 1: one sampler kernel, one marking kernel, one loss host path (rank_loss_run).  That case alone keeps two loss
// kernels of its own, bpr_slot_kernel and bpr_chunk_kernel, because they are faster there.
#include "refsum.hpp"
#include <cmath>

namespace {

constexpr int kBlock = 256;

// ------------------------------------------------------------------ sampler ------------
// Domain tags keep the edge-pick stream and the negative stream apart.
constexpr uint32_t kTagEdge = 0x45444745u;  // "EDGE"
constexpr uint32_t kTagNeg = 0x4E454721u;   // "NEG!"
constexpr int kMaxNegAttempts = 4096;

__device__ __forceinline__ bool csr_contains(const int32_t* __restrict__ rowptr,
                                             const int32_t* __restrict__ col, int64_t r,
                                             int32_t key) {
    int32_t lo = rowptr[r], hi = rowptr[r + 1];
    const int32_t end = hi;
    while (lo < hi) {
        int32_t mid = (lo + hi) >> 1;
        if (col[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo < end && col[lo] == key;
}

// One sampler kernel for the three entries, one thread per (slot, m).  Slot b takes edge e from the EDGE stream, counter
// (b); negative m of edge e, attempt t, takes the counter (e, t | m << 16) of the NEG! stream (t < 4096 < 2^16), so users,
// pos and column 0 of neg do not depend on n_neg, and the same edge drawn twice in a step gets the same negatives.  Draw
// says how the 64-bit word becomes a candidate and which candidates are redrawn beyond the user's own items:
//   modulus()      the word is reduced mod this; 0 = nothing to draw from, negative 0 for every slot
//   candidate(x)   the item of x in [0, modulus)
//   also_rejected  the draw's own rejection rules
struct UniformDraw {   // mi_sample_bpr_batch, mi_sample_bpr_batch_ex: x is the item; the two quirk bits of the header
    int64_t neg_range;
    int32_t quirk;
    __device__ uint64_t modulus() const { return (uint64_t)neg_range; }
    __device__ int32_t candidate(uint64_t x) const { return (int32_t)x; }
    __device__ bool also_rejected(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t u,
                                  int32_t cand) const {
        // reference key collision: (u-1, item neg_range) aliases (u, 0) in row*num_nodes+col
        if ((quirk & 1) && cand == 0 && u > 0 && csr_contains(rowptr, col, u - 1, (int32_t)neg_range)) return true;
        // contains_neg_self_loops=False: the key u*num_nodes+u of every node u < num_nodes is in the rejection set too
        return (quirk & 2) && (int64_t)cand == u;
    }
};

// Popularity-weighted negatives (mi_sample_bpr_batch_pop): the word is reduced mod total = cum[n_items - 1] and the
// candidate is the smallest i with cum[i] > x, by bisection over cum in global memory (ceil(log2 n_items) dependent loads;
// 400 KB at 100 K items).  x < total = cum[n_items - 1], so the answer exists and lies in [lo, hi] throughout; items of
// weight 0 have cum[i] == cum[i - 1] (or 0 at i = 0) and can never be the SMALLEST index above x.
struct PopularityDraw {
    int32_t n_items;
    const uint32_t* __restrict__ cum;
    __device__ uint64_t modulus() const { return cum[n_items - 1]; }
    __device__ int32_t candidate(uint64_t x) const {
        int32_t lo = 0, hi = n_items - 1;
        while (lo < hi) {
            const int32_t mid = lo + ((hi - lo) >> 1);
            if (cum[mid] > (uint32_t)x) hi = mid; else lo = mid + 1;
        }
        return lo;
    }
    __device__ bool also_rejected(const int32_t*, const int32_t*, int64_t, int32_t) const { return false; }
};

template <class Draw>
__global__ void sample_batch_kernel(int64_t batch, int n_neg, int64_t nnz, const int32_t* __restrict__ rowptr,
                                    const int32_t* __restrict__ col, const int32_t* __restrict__ row_of_edge, Draw draw,
                                    int32_t edges_in_order, uint64_t seed, uint64_t step, int64_t* __restrict__ users,
                                    int64_t* __restrict__ pos, int64_t* __restrict__ neg) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= batch * n_neg) return;
    const int64_t b = i / n_neg;
    const uint32_t m = (uint32_t)(i - b * n_neg);
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    const uint32_t s0 = (uint32_t)step, s1 = (uint32_t)(step >> 32);
    MiPhilox r = mi_philox4x32((uint32_t)b, (uint32_t)((uint64_t)b >> 32), s0, s1 ^ kTagEdge, k0, k1);
    const uint64_t e = edges_in_order ? (uint64_t)b : (((uint64_t)r.c[0] << 32) | r.c[1]) % (uint64_t)nnz;
    const int64_t u = row_of_edge[e];
    const uint64_t mod = draw.modulus();
    int32_t cand = 0;
    for (int t = 0; mod != 0 && t < kMaxNegAttempts; ++t) {
        MiPhilox q = mi_philox4x32((uint32_t)e, (uint32_t)t | (m << 16), s0, s1 ^ kTagNeg, k0, k1);
        cand = draw.candidate((((uint64_t)q.c[0] << 32) | q.c[1]) % mod);
        if (!csr_contains(rowptr, col, u, cand) && !draw.also_rejected(rowptr, col, u, cand)) break;
    }
    if (m == 0) {
        users[b] = u;
        pos[b] = col[e];
    }
    neg[i] = cand;
}

// ------------------------------------------------------------------ BPR ----------------
__device__ __forceinline__ float softplus_ref(float x) {  // torch softplus, beta=1, threshold=20
    return x > 20.f ? x : log1pf(expf(x));
}
__device__ __forceinline__ float softplus_grad_ref(float x) {  // torch softplus_backward
    if (x > 20.f) return 1.f;
    float z = expf(x);
    return z / (z + 1.f);
}

// The slot pass of (reference, M = 1, no logq), the default step: rank_slot_kernel's sums in the same order with one
// coefficient per slot, coef[b] = g_scale * dL/dx_b, for bpr_chunk_kernel.  It and bpr_chunk_kernel are kept beside the
// general kernels because those are slower at M = 1 (profiles/objectives.md section 5: 19.0 + 62.2 us against 17.4 + 41.3 us
// at B = 16 384, D = 128); rank_loss_run picks them, whichever entry was called.
// One wavefront per batch slot.  Each lane covers d/64 (rounded up) strided elements.
__global__ __launch_bounds__(kBlock) void bpr_slot_kernel(
    int64_t batch, int d, int64_t n_users, const int64_t* __restrict__ users,
    const int64_t* __restrict__ pos, const int64_t* __restrict__ neg,
    const float* __restrict__ fin, int64_t ldf, const float* __restrict__ e0, int64_t lde,
    float inv_batch, float g_scale, float reg_coef /* = lambda*reg_scale */,
    float* __restrict__ softplus_out, float* __restrict__ reg_out,
    float* __restrict__ coef_out, float* __restrict__ reg_w /* only when no gradient pass follows */,
    const int32_t* __restrict__ node_map) {
    const int64_t b = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / MI_WAVE;
    if (b >= batch) return;
    const int lane = mi_lane();
    const int64_t u = users[b], p = n_users + pos[b], n = n_users + neg[b];
    // rows of final / g_final: node ids, or compact slots when the batch-node map is given
    const int64_t fu = node_map ? node_map[u] : u, fp = node_map ? node_map[p] : p, fn = node_map ? node_map[n] : n;
    const float* uf = fin + fu * ldf;
    const float* pf = fin + fp * ldf;
    const float* nf = fin + fn * ldf;
    const float* u0 = e0 + u * lde;
    const float* p0 = e0 + p * lde;
    const float* n0 = e0 + n * lde;
    float sp = 0.f, sn = 0.f, rg = 0.f;
    for (int k = lane; k < d; k += MI_WAVE) {
        float a = uf[k];
        sp = fmaf(a, pf[k], sp);
        sn = fmaf(a, nf[k], sn);
        float x0 = u0[k], x1 = p0[k], x2 = n0[k];
        rg = fmaf(x0, x0, rg);
        rg = fmaf(x1, x1, rg);
        rg = fmaf(x2, x2, rg);
    }
    sp = mi_wave_sum(sp);
    sn = mi_wave_sum(sn);
    rg = mi_wave_sum(rg);
    const float x = sp - sn;
    if (lane == 0) {
        softplus_out[b] = softplus_ref(x);
        reg_out[b] = rg;
    }
    if (coef_out && lane == 0) {
        // loss = -mean softplus(x)  =>  dL/dx = -sigmoid'(x)/B; consumed by the segmented gradient kernels below
        coef_out[b] = -softplus_grad_ref(x) * inv_batch * g_scale;
    }
    // (with a gradient pass the weights come from the sorted references instead, bpr_chunk_kernel: the atomics of the few
    // hundred samples that share the most popular item serialised on one address — 49 of this kernel's 65 us at B = 16 384)
    if (reg_w && lane == 0) {
        const float w = 2.0f * reg_coef;
        atomicAdd(reg_w + u, w);
        atomicAdd(reg_w + p, w);
        atomicAdd(reg_w + n, w);
    }
}

// ---- gradient of the final embeddings, without float atomics -------------------------------------------------
// A batch touches (2 + M) B rows with repeats (the most popular item is the positive of hundreds of samples).  The
// (2 + M) B references (sample b, role) are keyed by the row they touch — its compact slot under node_map, its node id
// otherwise — by rank_refs_kernel, sorted (stable: the references of a row stay in (role, b) order) and summed row by row
// by the wave-per-chunk scheme of refsum.hpp.  The two chunk kernels below say what a reference adds.
constexpr int kMaxDPerLane = 8;  // d <= 512

// The chunk pass of (reference, M = 1, no logq), 3B references: a reference has at most two terms (the user's row takes
// p - n), so the lane that holds a reference holds its terms and the in-order pass needs no term numbering.
struct BprTerms {
    static constexpr int kTerms = 2;
    int64_t srcA = 0, srcB = 0;   // rows of final
    float wA = 0.f, wB = 0.f;     // wB == 0: one term
    __device__ __forceinline__ int64_t row(int t, int q) const { return __shfl(t == 0 ? srcA : srcB, q, MI_WAVE); }
    __device__ __forceinline__ float weight(int t, int q) const { return __shfl(t == 0 ? wA : wB, q, MI_WAVE); }
};

template <int VPT>  // floats of a row per lane: ceil(d / 64)
__global__ __launch_bounds__(kBlock) void bpr_chunk_kernel(
    int64_t batch, int64_t n_users, const int64_t* __restrict__ users, const int64_t* __restrict__ pos,
    const int64_t* __restrict__ neg, const float* __restrict__ fin, int64_t ldf, const float* __restrict__ coef,
    const uint32_t* __restrict__ keys, const uint32_t* __restrict__ refs, const int32_t* __restrict__ node_map,
    refsum::Dest to, float* __restrict__ reg_w, float reg_unit /* 2 * lambda * reg_scale: one reference's share */) {
    const int64_t n_ref = 3 * batch;
    const refsum::Chunk c = refsum::open_chunk(keys, n_ref);
    if (c.n_here == 0) return;
    BprTerms term;
    if (c.lane < c.n_here) {
        const uint32_t r = refs[c.j0 + c.lane];
        const int role = (int)(r / batch);
        const int64_t b = r - (int64_t)role * batch;
        const float cf = coef[b];
        const int64_t u = users[b], p = n_users + pos[b], n = n_users + neg[b];
        const int64_t fu = node_map ? node_map[u] : u, fp = node_map ? node_map[p] : p, fn = node_map ? node_map[n] : n;
        if (role == 0) { term.srcA = fp; term.wA = cf; term.srcB = fn; term.wB = -cf; }   // d x / d u = p - n
        else if (role == 1) { term.srcA = fu; term.wA = cf; }
        else { term.srcA = fu; term.wA = -cf; }
        if (reg_w) {
            const int64_t len = refsum::run_length(keys, c.j0 + c.lane, n_ref);
            if (len) reg_w[role == 0 ? u : (role == 1 ? p : n)] = (float)len * reg_unit;
        }
    }
    refsum::walk_references<VPT>(c, term, fin, ldf, to);
}

// ------------------------------------------------------------------ ranking objectives, M negatives ------------
// mi_rank_loss_fwd_bwd_f32: the same three passes as above over users[B], pos[B], neg[B, M].
//   x_{b,m} = s+_b - s-_{b,m};  reference: -softplus(x) / (BM);  bpr: softplus(-x) / (BM);
//   softmax: (logsumexp(s+_b, s-_{b,1..M}) - s+_b) / B
// The slot pass leaves 1 + M coefficients per slot for the gradient pass, coef[b][0] = g_scale * dL/ds+_b and
// coef[b][1 + m] = g_scale * dL/ds-_{b,m}.  At (reference, M = 1) every sum below runs in the order of the kernels above.
constexpr int kRankReference = 0, kRankBpr = 1, kRankSoftmax = 2;
constexpr int kMaxNeg = 16;

__device__ __forceinline__ float softplus_stable(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }
__device__ __forceinline__ float sigmoid_stable(float x) {
    const float z = expf(-fabsf(x));
    return (x >= 0.f ? 1.f : z) / (1.f + z);
}

// One wavefront per batch slot; the user's final row stays in registers (VPT = ceil(d / 64) floats per lane) while the
// positive and the M negatives stream past it.  Lane m keeps s-_{b,m}: scalars only, nothing indexed by m.
// LQ (mi_rank_loss_fwd_bwd_lq_f32, softmax only): the logits are s+_b - logq[pos_b] and s-_{b,m} - logq[neg_{b,m}], one
// fp32 subtraction each after the wave sums; LQ = false compiles to the kernel of before.
template <int VPT, bool LQ>
__global__ __launch_bounds__(kBlock) void rank_slot_kernel(
    int64_t batch, int n_neg, int objective, int d, int64_t n_users, const int64_t* __restrict__ users,
    const int64_t* __restrict__ pos, const int64_t* __restrict__ neg, const float* __restrict__ fin, int64_t ldf,
    const float* __restrict__ e0, int64_t lde, float inv_count, float g_scale, float reg_coef,
    float* __restrict__ term_out /* minus the slot's loss term, before the mean */, float* __restrict__ reg_out,
    float* __restrict__ coef_out, float* __restrict__ reg_w /* only when no gradient pass follows */,
    const int32_t* __restrict__ node_map, const float* __restrict__ logq /* [n_items], by item id; LQ only */) {
    const int64_t b = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / MI_WAVE;
    if (b >= batch) return;
    const int lane = mi_lane();
    const int64_t u = users[b], p = n_users + pos[b];
    const float* uf_row = fin + (node_map ? (int64_t)node_map[u] : u) * ldf;
    const float* pf_row = fin + (node_map ? (int64_t)node_map[p] : p) * ldf;
    const float* u0 = e0 + u * lde;
    const float* p0 = e0 + p * lde;
    float uf[VPT];
    float sp = 0.f, rg = 0.f;
#pragma unroll
    for (int v = 0; v < VPT; ++v) {
        const int k = lane + v * MI_WAVE;
        uf[v] = k < d ? uf_row[k] : 0.f;
        sp = fmaf(uf[v], k < d ? pf_row[k] : 0.f, sp);
    }
    sp = mi_wave_sum(sp);
    float my_sn = 0.f;
    for (int m = 0; m < n_neg; ++m) {
        const int64_t n = n_users + neg[b * n_neg + m];
        const float* nf_row = fin + (node_map ? (int64_t)node_map[n] : n) * ldf;
        const float* n0 = e0 + n * lde;
        float sn = 0.f;
#pragma unroll
        for (int v = 0; v < VPT; ++v) {
            const int k = lane + v * MI_WAVE;
            const bool in = k < d;
            sn = fmaf(uf[v], in ? nf_row[k] : 0.f, sn);
            if (m == 0) {   // |u0|^2 and |p0|^2 once, interleaved with the first negative's as in bpr_slot_kernel
                const float x0 = in ? u0[k] : 0.f, x1 = in ? p0[k] : 0.f;
                rg = fmaf(x0, x0, rg);
                rg = fmaf(x1, x1, rg);
            }
            const float x2 = in ? n0[k] : 0.f;
            rg = fmaf(x2, x2, rg);
        }
        sn = mi_wave_sum(sn);
        if (lane == m) my_sn = sn;
    }
    rg = mi_wave_sum(rg);
    const bool mine = lane < n_neg;
    if (LQ) {   // constant per logit: the coefficient formulas below keep their form
        sp -= logq[pos[b]];
        if (mine) my_sn -= logq[neg[b * n_neg + lane]];
    }
    float term, a, dm;   // term: wave-uniform; a = coef[b][0]: wave-uniform; dm = coef[b][1 + lane]
    if (objective == kRankSoftmax) {
        float mx = sp;
        for (int m = 0; m < n_neg; ++m) mx = fmaxf(mx, __shfl(my_sn, m, MI_WAVE));
        const float ep = expf(sp - mx);
        const float en = mine ? expf(my_sn - mx) : 0.f;
        float sum = ep;
        for (int m = 0; m < n_neg; ++m) sum += __shfl(en, m, MI_WAVE);   // ascending m
        term = -((mx + logf(sum)) - sp);
        const float w = inv_count * g_scale;
        a = (ep / sum - 1.f) * w;
        dm = (en / sum) * w;
    } else {
        const float x = sp - my_sn;
        float val, c;   // c = g_scale * dL/dx_{b,lane}
        if (objective == kRankReference) {
            val = softplus_ref(x);
            c = -softplus_grad_ref(x) * inv_count * g_scale;
        } else {
            val = -softplus_stable(-x);
            c = -sigmoid_stable(-x) * inv_count * g_scale;
        }
        term = __shfl(val, 0, MI_WAVE);
        a = __shfl(c, 0, MI_WAVE);
        for (int m = 1; m < n_neg; ++m) {   // ascending m
            term += __shfl(val, m, MI_WAVE);
            a += __shfl(c, m, MI_WAVE);
        }
        dm = -c;
    }
    if (lane == 0) {
        term_out[b] = term;
        reg_out[b] = rg;
    }
    if (coef_out) {
        float* cb = coef_out + b * (1 + n_neg);
        if (lane == 0) cb[0] = a;
        if (mine) cb[1 + lane] = dm;
    }
    if (reg_w) {
        const float w = 2.0f * reg_coef;
        if (lane == 0) {
            atomicAdd(reg_w + u, w);
            atomicAdd(reg_w + p, w);
        }
        if (mine) atomicAdd(reg_w + n_users + neg[b * n_neg + lane], w);
    }
}

__global__ void rank_refs_kernel(int64_t batch, int n_neg, int64_t n_users, const int64_t* __restrict__ users,
                                 const int64_t* __restrict__ pos, const int64_t* __restrict__ neg,
                                 const int32_t* __restrict__ node_map, uint32_t* __restrict__ keys,
                                 uint32_t* __restrict__ refs) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // reference id = role * batch + b
    if (r >= (2 + n_neg) * batch) return;
    const int role = (int)(r / batch);   // 0 user, 1 positive, 2 + m negative m
    const int64_t b = r - role * batch;
    const int64_t node = role == 0 ? users[b] : n_users + (role == 1 ? pos[b] : neg[b * n_neg + (role - 2)]);
    keys[r] = (uint32_t)(node_map ? node_map[node] : node);
    refs[r] = (uint32_t)r;
}

// bpr_chunk_kernel for (2 + M) B references.  A user reference carries 1 + M (source row, weight) terms — the positive,
// then the negatives in order — an item reference one.  The terms of a chunk are numbered through (wave prefix sum of the
// per-reference counts) and taken in rounds of 64, lane L preparing term r0 + L; the in-order pass then keeps U source rows
// in flight whatever the mix of roles.
template <int VPT>
__global__ __launch_bounds__(kBlock) void rank_chunk_kernel(
    int64_t batch, int n_neg, int64_t n_users, const int64_t* __restrict__ users,
    const int64_t* __restrict__ pos, const int64_t* __restrict__ neg, const float* __restrict__ fin, int64_t ldf,
    const float* __restrict__ coef, const uint32_t* __restrict__ keys, const uint32_t* __restrict__ refs,
    const int32_t* __restrict__ node_map, refsum::Dest to, float* __restrict__ reg_w, float reg_unit) {
    const int64_t n_ref = (2 + n_neg) * batch;
    const refsum::Chunk c = refsum::open_chunk(keys, n_ref);
    if (c.n_here == 0) return;
    const int lane = c.lane, n_here = c.n_here;
    int my_role = 1, my_b = 0, my_terms = 0;
    if (lane < n_here) {
        const uint32_t r = refs[c.j0 + lane];
        my_role = (int)(r / batch);
        my_b = (int)(r - (int64_t)my_role * batch);
        my_terms = my_role == 0 ? 1 + n_neg : 1;
        if (reg_w) {
            const int64_t len = refsum::run_length(keys, c.j0 + lane, n_ref);
            if (len) {
                const int64_t node = my_role == 0 ? users[my_b] : n_users + (my_role == 1 ? pos[my_b] : neg[(int64_t)my_b * n_neg + (my_role - 2)]);
                reg_w[node] = (float)len * reg_unit;
            }
        }
    }
    int incl = my_terms;   // inclusive prefix sum over the wavefront
#pragma unroll
    for (int off = 1; off < MI_WAVE; off <<= 1) {
        const int below = __shfl_up(incl, off, MI_WAVE);
        if (lane >= off) incl += below;
    }
    const int total = __shfl(incl, MI_WAVE - 1, MI_WAVE);
    const int excl = incl - my_terms;
    refsum::RunWriter<VPT> run;
    constexpr int U = refsum::kInFlight;  // terms whose source rows are in flight together
    for (int r0 = 0; r0 < total; r0 += MI_WAVE) {
        // a round of up to 64 terms, one per lane: owner by bisection over the prefix sums, then this lane's own chain of
        // loads (ids -> slot -> weight), so that the in-order pass below only shuffles
        const int n_round = min(MI_WAVE, total - r0);
        const int j = min(r0 + lane, total - 1);
        // owner of term j = the q with incl[q - 1] <= j < incl[q] (incl[-1] = 0): the smallest q with incl[q] > j.  It lies in
        // [lo, hi] throughout — incl[n_here - 1] = total > j, so hi always satisfies the test — and each step halves that
        // range of at most 64 references: 6 steps leave lo == hi.  Every lane runs all 6 (the shuffles need the whole wave).
        int lo = 0, hi = n_here - 1;
#pragma unroll
        for (int it = 0; it < 6; ++it) {
            const int mid = (lo + hi) >> 1;
            if (__shfl(incl, mid, MI_WAVE) > j) hi = mid; else lo = mid + 1;
        }
        const int t_owner = hi;
        const int role = __shfl(my_role, t_owner, MI_WAVE);
        const int64_t b = __shfl(my_b, t_owner, MI_WAVE);
        const int tt = j - __shfl(excl, t_owner, MI_WAVE);
        const int t_closes = j + 1 == __shfl(incl, t_owner, MI_WAVE);
        int64_t t_src;
        int ci;
        if (role == 0) {
            t_src = n_users + (tt == 0 ? pos[b] : neg[b * n_neg + (tt - 1)]);
            ci = tt;
        } else {
            t_src = users[b];
            ci = role - 1;
        }
        if (node_map) t_src = node_map[t_src];
        const float t_w = r0 + lane < total ? coef[b * (1 + n_neg) + ci] : 0.f;
        for (int q0 = 0; q0 < n_round; q0 += U) {
            float x[U][VPT], w[U];
#pragma unroll
            for (int i = 0; i < U; ++i) {
                const int sl = min(q0 + i, n_round - 1);
                const bool live = q0 + i < n_round;
                w[i] = live ? __shfl(t_w, sl, MI_WAVE) : 0.f;
                const float* row = fin + __shfl(t_src, sl, MI_WAVE) * ldf;
#pragma unroll
                for (int v = 0; v < VPT; ++v) {
                    const int k = lane + v * MI_WAVE;
                    x[i][v] = (live && k < to.d) ? row[k] : 0.f;
                }
            }
#pragma unroll
            for (int i = 0; i < U; ++i) {
                const int sl = q0 + i;
                if (sl >= n_round) break;
                run.add(w[i], x[i]);
                if (!__shfl(t_closes, sl, MI_WAVE)) continue;   // more terms of this reference follow
                run.close(c, __shfl(t_owner, sl, MI_WAVE), to);
            }
        }
    }
}

// ------------------------------------------------------------------ batch node set ------
__global__ void mark_batch_nodes_ex_kernel(int64_t batch, int n_neg, int64_t n_users, const int64_t* __restrict__ users,
                                           const int64_t* __restrict__ pos, const int64_t* __restrict__ neg,
                                           int32_t* __restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // (slot, m)
    if (i >= batch * n_neg) return;
    flag[n_users + neg[i]] = 1;  // same value from every writer: order does not matter
    if (i % n_neg == 0) {
        const int64_t b = i / n_neg;
        flag[users[b]] = 1;
        flag[n_users + pos[b]] = 1;
    }
}

__global__ void finish_batch_nodes_kernel(int64_t n_nodes, int64_t n_users, const int32_t* __restrict__ flag,
                                          const int32_t* __restrict__ slot, int32_t* __restrict__ gmap,
                                          int32_t* __restrict__ nodes, int32_t* __restrict__ count) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n_nodes) return;
    if (r == n_users) count[1] = slot[r];  // unique USER nodes: slots [0, count[1]) are users, the rest items
    if (r == n_nodes) {
        count[0] = slot[r];
        return;
    }
    if (flag[r]) {
        gmap[r] = slot[r];
        nodes[slot[r]] = (int32_t)r;
    } else {
        gmap[r] = -1;
    }
}

// dst[i,:] = scale * ((accumulate ? dst[i,:] : 0) + src[rows[i] - row_offset,:]) for i in [*begin_dev, *n_dev);
// one wavefront per row, float4 lanes
__global__ __launch_bounds__(kBlock) void gather_rows_kernel(int64_t n_max, const int32_t* __restrict__ n_dev,
                                                             const int32_t* __restrict__ begin_dev,
                                                             int d4, const int32_t* __restrict__ rows,
                                                             int64_t row_offset,
                                                             const float4* __restrict__ src, int64_t lds4,
                                                             float4* __restrict__ dst, int64_t ldd4, int accumulate,
                                                             float scale) {
    const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / MI_WAVE;
    if (i >= n_max || (n_dev && i >= *n_dev) || (begin_dev && i < *begin_dev)) return;
    const int64_t r = (int64_t)rows[i] - row_offset;
    for (int e = mi_lane(); e < d4; e += MI_WAVE) {
        float4 v = src[r * lds4 + e];
        if (accumulate) v = mi_f4_add(dst[i * ldd4 + e], v);
        if (scale != 1.0f) { v.x *= scale; v.y *= scale; v.z *= scale; v.w *= scale; }
        dst[i * ldd4 + e] = v;
    }
}

// dst[rows[i] - row_offset,:] = src[i,:] for i in [*begin_dev, *n_dev): the inverse of gather_rows (rows are distinct)
__global__ __launch_bounds__(kBlock) void scatter_rows_kernel(int64_t n_max, const int32_t* __restrict__ n_dev,
                                                              const int32_t* __restrict__ begin_dev, int d4,
                                                              const int32_t* __restrict__ rows, int64_t row_offset,
                                                              const float4* __restrict__ src, int64_t lds4,
                                                              float4* __restrict__ dst, int64_t ldd4) {
    const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / MI_WAVE;
    if (i >= n_max || (n_dev && i >= *n_dev) || (begin_dev && i < *begin_dev)) return;
    const int64_t r = (int64_t)rows[i] - row_offset;
    for (int e = mi_lane(); e < d4; e += MI_WAVE) dst[r * ldd4 + e] = src[i * lds4 + e];
}

// ------------------------------------------------------------------ Adam ---------------
// One wavefront per group of rows: lane -> (row within group, float4 column), so the row index (needed
// for the L2 weight) costs no integer division, and every lane keeps 4 independent 16-byte loads in flight.
__global__ __launch_bounds__(kBlock) void adam_kernel(int64_t n_rows, int d4, float4* __restrict__ p,
                                                      int64_t ldp4, const float4* __restrict__ g,
                                                      int64_t ldg4, float4* __restrict__ m,
                                                      float4* __restrict__ v,
                                                      const float* __restrict__ reg_w, MiAdamConsts c) {
    // rows per pass of one block: blockDim.x / lanes-per-row, lanes-per-row = smallest power of two >= d4 (<= 256)
    int lpr = 1;
    while (lpr < d4 && lpr < (int)blockDim.x) lpr <<= 1;
    const int rows_per_block = blockDim.x / lpr;
    const int sub = threadIdx.x / lpr, e0 = threadIdx.x % lpr;
    for (int64_t r = (int64_t)blockIdx.x * rows_per_block + sub; r < n_rows; r += (int64_t)gridDim.x * rows_per_block) {
        const float w = reg_w ? reg_w[r] : 0.f;
        for (int e = e0; e < d4; e += lpr) {
            const int64_t i = r * d4 + e;
            float4 pp = p[r * ldp4 + e];
            float4 mm = m[i];
            float4 vv = v[i];
            mi_adam_update4(pp, g[r * ldg4 + e], mm, vv, reg_w != nullptr, w, c);
            p[r * ldp4 + e] = pp;
            m[i] = mm;
            v[i] = vv;
        }
    }
}

// ------------------------------------------------------------------ host helpers -------
template <class Draw>   // arguments checked by the caller; batch * n_neg >= 1
int sample_batch_launch(int64_t batch, int n_neg, int64_t nnz, const int32_t* rowptr, const int32_t* col,
                        const int32_t* row_of_edge, Draw draw, int32_t edges_in_order, uint64_t seed, uint64_t step,
                        int64_t* users, int64_t* pos, int64_t* neg, mi_stream_t stream) {
    hipLaunchKernelGGL(sample_batch_kernel<Draw>, dim3((unsigned)mi_ceil_div(batch * n_neg, kBlock)), dim3(kBlock), 0,
                       (hipStream_t)stream, batch, n_neg, nnz, rowptr, col, row_of_edge, draw, edges_in_order, seed, step,
                       users, pos, neg);
    return mi_launch_status();
}

}  // namespace

extern "C" {

int mi_sample_bpr_batch_ex(int64_t batch, int32_t n_neg, int64_t nnz, const int32_t* rowptr, const int32_t* col,
                           const int32_t* row_of_edge, int64_t neg_range, int32_t quirk_user_rows,
                           int32_t edges_in_order, uint64_t seed, uint64_t step, int64_t* users, int64_t* pos,
                           int64_t* neg, mi_stream_t stream) {
    if (n_neg < 1 || n_neg > kMaxNeg) return MI_ERR_UNSUPPORTED;
    MI_CHECK_ARG(batch >= 0 && (!edges_in_order || batch <= nnz));
    if (batch == 0) return 0;
    MI_CHECK_ARG(nnz > 0 && neg_range > 0 && rowptr && col && row_of_edge && users && pos && neg);
    if (nnz >= INT32_MAX || neg_range >= INT32_MAX) return MI_ERR_TOO_LARGE;
    return sample_batch_launch(batch, n_neg, nnz, rowptr, col, row_of_edge, UniformDraw{neg_range, quirk_user_rows},
                               edges_in_order, seed, step, users, pos, neg, stream);
}

// the one-negative form: same checks, same kernel, n_neg = 1
int mi_sample_bpr_batch(int64_t batch, int64_t nnz, const int32_t* rowptr, const int32_t* col,
                        const int32_t* row_of_edge, int64_t neg_range, int32_t quirk_user_rows,
                        int32_t edges_in_order, uint64_t seed, uint64_t step, int64_t* users, int64_t* pos,
                        int64_t* neg, mi_stream_t stream) {
    return mi_sample_bpr_batch_ex(batch, 1, nnz, rowptr, col, row_of_edge, neg_range, quirk_user_rows, edges_in_order, seed,
                                  step, users, pos, neg, stream);
}

int mi_sample_bpr_batch_pop(int64_t batch, int32_t n_neg, int64_t nnz, const int32_t* rowptr, const int32_t* col,
                            const int32_t* row_of_edge, int64_t n_items, const uint32_t* cum, int32_t edges_in_order,
                            uint64_t seed, uint64_t step, int64_t* users, int64_t* pos, int64_t* neg, mi_stream_t stream) {
    if (n_neg > kMaxNeg) return MI_ERR_UNSUPPORTED;
    MI_CHECK_ARG(n_neg >= 1 && batch >= 1 && nnz >= 1 && n_items >= 1 && (!edges_in_order || batch <= nnz));
    MI_CHECK_ARG(rowptr && col && row_of_edge && cum && users && pos && neg);
    MI_CHECK_ARG(((uintptr_t)rowptr | (uintptr_t)col | (uintptr_t)row_of_edge | (uintptr_t)cum) % 4 == 0);
    MI_CHECK_ARG(((uintptr_t)users | (uintptr_t)pos | (uintptr_t)neg) % 8 == 0);
    if (nnz >= INT32_MAX || n_items > INT32_MAX) return MI_ERR_TOO_LARGE;
    return sample_batch_launch(batch, n_neg, nnz, rowptr, col, row_of_edge, PopularityDraw{(int32_t)n_items, cum},
                               edges_in_order, seed, step, users, pos, neg, stream);
}

size_t mi_batch_nodes_workspace_bytes(int64_t n_nodes) {
    const size_t n1 = (size_t)(n_nodes > 0 ? n_nodes : 0) + 1;
    return 2 * mi_align_up(n1 * sizeof(int32_t), 256) + ((size_t)16 << 20);
}

static int batch_nodes_run(int64_t batch, int n_neg, int64_t n_users, int64_t n_nodes, const int64_t* users,
                           const int64_t* pos, const int64_t* neg, int32_t* gmap, int32_t* nodes,
                           int32_t* count, void* ws, size_t ws_bytes, mi_stream_t stream) {
    MI_CHECK_ARG(batch > 0 && n_users >= 0 && n_nodes >= n_users && n_nodes > 0);
    MI_CHECK_ARG(users && pos && neg && gmap && nodes && count && ws);
    if (n_nodes >= INT32_MAX) return MI_ERR_TOO_LARGE;
    hipStream_t s = (hipStream_t)stream;
    const int64_t n1 = n_nodes + 1;
    MiArena arena(ws, ws_bytes);
    int32_t* flag = arena.take<int32_t>(n1);
    int32_t* slot = arena.take<int32_t>(n1);
    if (!flag || !slot) return MI_ERR_WORKSPACE;
    MI_HIP(hipMemsetAsync(flag, 0, (size_t)n1 * sizeof(int32_t), s));
    hipLaunchKernelGGL(mark_batch_nodes_ex_kernel, dim3((unsigned)mi_ceil_div(batch * n_neg, kBlock)), dim3(kBlock), 0, s,
                       batch, n_neg, n_users, users, pos, neg, flag);
    size_t tmp_bytes = 0;
    MI_HIP(rocprim::exclusive_scan(nullptr, tmp_bytes, flag, slot, 0, (size_t)n1, rocprim::plus<int32_t>(), s));
    char* tmp = arena.take<char>(tmp_bytes ? tmp_bytes : 1);
    if (!tmp) return MI_ERR_WORKSPACE;
    MI_HIP(rocprim::exclusive_scan(tmp, tmp_bytes, flag, slot, 0, (size_t)n1, rocprim::plus<int32_t>(), s));
    hipLaunchKernelGGL(finish_batch_nodes_kernel, dim3((unsigned)mi_ceil_div(n1, kBlock)), dim3(kBlock), 0, s, n_nodes,
                       n_users, flag, slot, gmap, nodes, count);
    return mi_launch_status();
}

int mi_batch_nodes_i32(int64_t batch, int64_t n_users, int64_t n_nodes, const int64_t* users,
                       const int64_t* pos, const int64_t* neg, int32_t* gmap, int32_t* nodes,
                       int32_t* count, void* ws, size_t ws_bytes, mi_stream_t stream) {
    return batch_nodes_run(batch, 1, n_users, n_nodes, users, pos, neg, gmap, nodes, count, ws, ws_bytes, stream);
}

int mi_batch_nodes_ex_i32(int64_t batch, int32_t n_neg, int64_t n_users, int64_t n_nodes, const int64_t* users,
                          const int64_t* pos, const int64_t* neg, int32_t* gmap, int32_t* nodes,
                          int32_t* count, void* ws, size_t ws_bytes, mi_stream_t stream) {
    if (n_neg < 1 || n_neg > kMaxNeg) return MI_ERR_UNSUPPORTED;
    return batch_nodes_run(batch, n_neg, n_users, n_nodes, users, pos, neg, gmap, nodes, count, ws, ws_bytes, stream);
}

int mi_gather_rows_f32(int64_t n_max, const int32_t* n_dev, const int32_t* begin_dev, int64_t d,
                       const int32_t* rows, int64_t row_offset, const float* src, int64_t ld_src, float* dst,
                       int64_t ld_dst, int32_t accumulate, float scale, mi_stream_t stream) {
    MI_CHECK_ARG(n_max >= 0 && d > 0);
    if (n_max == 0) return 0;
    if (d % 4 != 0) return MI_ERR_UNSUPPORTED;
    MI_CHECK_ARG(rows && src && dst && ld_src % 4 == 0 && ld_dst % 4 == 0 && ld_src >= d && ld_dst >= d);
    MI_CHECK_ARG(mi_aligned16(src) && mi_aligned16(dst));
    hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)mi_ceil_div(n_max * MI_WAVE, kBlock)), dim3(kBlock), 0,
                       (hipStream_t)stream, n_max, n_dev, begin_dev, (int)(d / 4), rows, row_offset,
                       reinterpret_cast<const float4*>(src), ld_src / 4, reinterpret_cast<float4*>(dst), ld_dst / 4,
                       accumulate, scale);
    return mi_launch_status();
}

int mi_scatter_rows_f32(int64_t n_max, const int32_t* n_dev, const int32_t* begin_dev, int64_t d,
                        const int32_t* rows, int64_t row_offset, const float* src, int64_t ld_src, float* dst,
                        int64_t ld_dst, mi_stream_t stream) {
    MI_CHECK_ARG(n_max >= 0 && d > 0);
    if (n_max == 0) return 0;
    if (d % 4 != 0) return MI_ERR_UNSUPPORTED;
    MI_CHECK_ARG(rows && src && dst && ld_src % 4 == 0 && ld_dst % 4 == 0 && ld_src >= d && ld_dst >= d);
    MI_CHECK_ARG(mi_aligned16(src) && mi_aligned16(dst));
    hipLaunchKernelGGL(scatter_rows_kernel, dim3((unsigned)mi_ceil_div(n_max * MI_WAVE, kBlock)), dim3(kBlock), 0,
                       (hipStream_t)stream, n_max, n_dev, begin_dev, (int)(d / 4), rows, row_offset,
                       reinterpret_cast<const float4*>(src), ld_src / 4, reinterpret_cast<float4*>(dst), ld_dst / 4);
    return mi_launch_status();
}

size_t mi_rank_loss_workspace_bytes(int64_t batch, int32_t n_neg) {
    const size_t b = (size_t)(batch > 0 ? batch : 1);
    const size_t m = (size_t)(n_neg >= 1 && n_neg <= kMaxNeg ? n_neg : 1);
    // loss term, reg per slot; 1 + M coefficients per slot; the segmented sum's buffers.  This function is not told d, so the
    // partial rows are sized for the widest row the kernels take (d <= 512); the kernels address them d floats apart.
    return 2 * mi_align_up(b * sizeof(float), 256) + mi_align_up((1 + m) * b * sizeof(float), 256) +
           refsum::workspace_bytes((int64_t)((2 + m) * b), MI_WAVE * kMaxDPerLane);
}

// all three loss entries; logq == nullptr launches what mi_rank_loss_fwd_bwd_f32 always launched
static int rank_loss_run(int64_t batch, int32_t n_neg, int32_t objective, int64_t d, int64_t n_users,
                         const int64_t* users, const int64_t* pos, const int64_t* neg, const float* final_emb,
                         int64_t ldf, const float* e0, int64_t lde, float lambda, float g_scale, float reg_scale,
                         float* loss_out, float* g_final, int64_t ldg, float* reg_w, const int32_t* node_map,
                         const float* logq, void* ws, size_t ws_bytes, mi_stream_t stream) {
    if (n_neg < 1 || n_neg > kMaxNeg) return MI_ERR_UNSUPPORTED;
    if (objective != kRankReference && objective != kRankBpr && objective != kRankSoftmax) return MI_ERR_UNSUPPORTED;
    if (logq && objective != kRankSoftmax) return MI_ERR_UNSUPPORTED;
    // the loss-only form accumulates reg_w with float atomics in the slot pass: not on the corrected path
    if (logq && !g_final && reg_w) return MI_ERR_UNSUPPORTED;
    MI_CHECK_ARG(batch > 0 && d > 0 && n_users >= 0);
    MI_CHECK_ARG(users && pos && neg && final_emb && e0 && loss_out && ws);
    MI_CHECK_ARG(ldf >= d && lde >= d && (!g_final || ldg >= d));
    if ((2 + (int64_t)n_neg) * batch >= INT32_MAX) return MI_ERR_TOO_LARGE;
    if (d > MI_WAVE * kMaxDPerLane) return MI_ERR_UNSUPPORTED;
    if (ws_bytes < mi_rank_loss_workspace_bytes(batch, n_neg)) return MI_ERR_WORKSPACE;
    const int64_t n_ref = (2 + (int64_t)n_neg) * batch;
    MiArena arena(ws, ws_bytes);
    float* termv = arena.take<float>(batch);
    float* rgv = arena.take<float>(batch);
    float* coef = arena.take<float>((size_t)(1 + n_neg) * batch);
    const refsum::Buffers sum = refsum::take(arena, n_ref, MI_WAVE * kMaxDPerLane);
    if (!termv || !rgv || !coef || !sum.ok()) return MI_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    refsum::Sort sorted;
    if (g_final) {
        const int rc = refsum::plan_sort(sum, n_ref, node_map != nullptr, s, sorted);
        if (rc) return rc;
    }
    // ---- nothing has been enqueued up to here ----
    // the mean runs over the B*M pairs, or over the B slots for the softmax
    const float inv_count = 1.0f / (float)(objective == kRankSoftmax ? batch : batch * n_neg);
    const float reg_coef = reg_scale * lambda;
    // the default step's case keeps its two faster kernels (same bits; one coefficient per slot instead of two)
    const bool bpr_form = n_neg == 1 && objective == kRankReference && !logq;
    const dim3 g((unsigned)mi_ceil_div(batch * MI_WAVE, kBlock));
    float* const coef_out = g_final ? coef : nullptr;
    float* const slot_reg_w = g_final ? nullptr : reg_w;
    const int64_t vpt = mi_ceil_div(d, MI_WAVE);
    if (bpr_form)
        hipLaunchKernelGGL(bpr_slot_kernel, g, dim3(kBlock), 0, s, batch, (int)d, n_users, users, pos, neg, final_emb, ldf,
                           e0, lde, inv_count, g_scale, reg_coef, termv, rgv, coef_out, slot_reg_w, node_map);
    else
        refsum::with_vpt(vpt, [&](auto v) {
            constexpr int V = decltype(v)::value;
            auto slot = logq ? rank_slot_kernel<V, true> : rank_slot_kernel<V, false>;
            hipLaunchKernelGGL(slot, g, dim3(kBlock), 0, s, batch, (int)n_neg, (int)objective, (int)d, n_users, users, pos,
                               neg, final_emb, ldf, e0, lde, inv_count, g_scale, reg_coef, termv, rgv, coef_out, slot_reg_w,
                               node_map, logq);
        });
    if (g_final) {
        hipLaunchKernelGGL(rank_refs_kernel, dim3((unsigned)mi_ceil_div(n_ref, 256)), dim3(256), 0, s, batch, (int)n_neg,
                           n_users, users, pos, neg, node_map, sum.k0, sum.r0);
        const int rc = refsum::sort(sum, n_ref, s, sorted);
        if (rc) return rc;
        const uint32_t *keys = sorted.keys.current(), *refs = sorted.refs.current();
        const refsum::Dest to{g_final, ldg, sum.part_head, sum.part_tail, (int)d};
        const dim3 gc = refsum::chunk_grid(n_ref);
        refsum::with_vpt(vpt, [&](auto v) {
            constexpr int V = decltype(v)::value;
            if (bpr_form)
                hipLaunchKernelGGL(bpr_chunk_kernel<V>, gc, dim3(kBlock), 0, s, batch, n_users, users, pos, neg, final_emb,
                                   ldf, coef, keys, refs, node_map, to, reg_w, 2.0f * reg_coef);
            else
                hipLaunchKernelGGL(rank_chunk_kernel<V>, gc, dim3(kBlock), 0, s, batch, (int)n_neg, n_users, users, pos, neg,
                                   final_emb, ldf, coef, keys, refs, node_map, to, reg_w, 2.0f * reg_coef);
            refsum::launch_combine<V>(sorted, n_ref, to, s);
        });
    }
    // the slot terms are stored negated, so every objective closes with loss = -sum(term) / count + lambda * sum(reg)
    refsum::launch_finish(batch, termv, rgv, -inv_count, lambda, loss_out, s);
    return mi_launch_status();
}

int mi_rank_loss_fwd_bwd_f32(int64_t batch, int32_t n_neg, int32_t objective, int64_t d, int64_t n_users,
                             const int64_t* users, const int64_t* pos, const int64_t* neg, const float* final_emb,
                             int64_t ldf, const float* e0, int64_t lde, float lambda, float g_scale, float reg_scale,
                             float* loss_out, float* g_final, int64_t ldg, float* reg_w, const int32_t* node_map,
                             void* ws, size_t ws_bytes, mi_stream_t stream) {
    return rank_loss_run(batch, n_neg, objective, d, n_users, users, pos, neg, final_emb, ldf, e0, lde, lambda, g_scale,
                         reg_scale, loss_out, g_final, ldg, reg_w, node_map, nullptr, ws, ws_bytes, stream);
}

// the reference's loss: the (MI_RANK_REFERENCE, one negative) case, kept for the boundary
size_t mi_bpr_workspace_bytes(int64_t batch) { return mi_rank_loss_workspace_bytes(batch, 1); }

int mi_bpr_fwd_bwd_f32(int64_t batch, int64_t d, int64_t n_users, const int64_t* users,
                       const int64_t* pos, const int64_t* neg, const float* final_emb, int64_t ldf,
                       const float* e0, int64_t lde, float lambda, float g_scale, float reg_scale,
                       float* loss_out, float* g_final, int64_t ldg, float* reg_w,
                       const int32_t* node_map, void* ws, size_t ws_bytes, mi_stream_t stream) {
    return rank_loss_run(batch, 1, kRankReference, d, n_users, users, pos, neg, final_emb, ldf, e0, lde, lambda, g_scale,
                         reg_scale, loss_out, g_final, ldg, reg_w, node_map, nullptr, ws, ws_bytes, stream);
}

int mi_rank_loss_fwd_bwd_lq_f32(int64_t batch, int32_t n_neg, int32_t objective, int64_t d, int64_t n_users,
                                const int64_t* users, const int64_t* pos, const int64_t* neg, const float* final_emb,
                                int64_t ldf, const float* e0, int64_t lde, float lambda, float g_scale, float reg_scale,
                                float* loss_out, float* g_final, int64_t ldg, float* reg_w, const int32_t* node_map,
                                const float* logq, void* ws, size_t ws_bytes, mi_stream_t stream) {
    return rank_loss_run(batch, n_neg, objective, d, n_users, users, pos, neg, final_emb, ldf, e0, lde, lambda, g_scale,
                         reg_scale, loss_out, g_final, ldg, reg_w, node_map, logq, ws, ws_bytes, stream);
}

int mi_adam_dense_f32(int64_t n_rows, int64_t d, float* p, int64_t ldp, const float* grad,
                      int64_t ldgr, float* m, float* v, const float* reg_w, double lr, double beta1,
                      double beta2, double eps, int64_t step, mi_stream_t stream) {
    MI_CHECK_ARG(n_rows >= 0 && d > 0 && step >= 1);
    if (n_rows == 0) return 0;
    MI_CHECK_ARG(p && grad && m && v);
    if (d % 4 != 0) return MI_ERR_UNSUPPORTED;
    MI_CHECK_ARG(ldp % 4 == 0 && ldgr % 4 == 0 && ldp >= d && ldgr >= d);
    MI_CHECK_ARG(mi_aligned16(p) && mi_aligned16(grad) && mi_aligned16(m) && mi_aligned16(v));
    // scalar constants in double, as torch.optim.Adam derives them, then rounded once to fp32
    const MiAdamConsts c = mi_adam_consts(lr, beta1, beta2, eps, step);
    const int64_t total = n_rows * (d / 4);
    int64_t blocks = mi_ceil_div(total, kBlock);
    if (blocks > 256 * 32) blocks = 256 * 32;
    hipLaunchKernelGGL(adam_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, n_rows,
                       (int)(d / 4), reinterpret_cast<float4*>(p), ldp / 4,
                       reinterpret_cast<const float4*>(grad), ldgr / 4, reinterpret_cast<float4*>(m),
                       reinterpret_cast<float4*>(v), reg_w, c);
    return mi_launch_status();
}

}  // extern "C"
