// Noise-view contrastive regulariser of the LightGCN trainer (the rule is in the header, "Noise-view contrastive term").
//   mi_perturb_rows_f32         X[r, :] += eps * sign(X[r, :]) * n[r, :], n the unit vector of Philox uniforms keyed on
//                               (seed, step, layer, the row's ORIGINAL id); optionally S = (addend + X) * scale in the same pass.
//                               A sub-group of LPR lanes per row (LPR the power of two >= d / 4), one float4 and one Philox
//                               block per lane, the norm by xor shuffles inside the sub-group.  No atomics, one writer per row.
//   mi_contrastive_fwd_bwd_f32  InfoNCE between p_b = a[id_b] / |a[id_b]| and q_j = b[id_j] / |b[id_j]| over the groups of G
//                               slots of the in-batch softmax, whose row statistics and gradient sweeps (inbatch_tiles.hpp,
//                               on the score tiles of loss_tiles.hpp) it runs on two normalised [B, d] images: u_img = p / tau,
//                               v_img = q, both mask ids = id, no logit offset.
//     1. normalise_kernel   one wavefront per slot: the two rows, their norms, the images, the slot's sort key
//     2. inbatch_stats_kernel, 3. inbatch_sweep_kernel   as in inbatch.hip: lse and loss term per slot; dL/du_img, dL/dv_img
//     4. norm_bwd_kernel    one wavefront per slot row: through the normalisation, (I - p p^T) / |f|, times its side's scale
//     5. sort / chunk / combine   the slot rows of each side are summed per id by refsum.hpp and ADDED to g_a / g_b
//     6. refsum::finish_kernel    loss = sum(term) / B
// Every order of summation is a function of (B, G, d) and the ids: two calls give equal bits.
// This file owns the noise, the normalisation and its backward, and the host entries; the lane map, k order and rescale order
// of the scores are written in loss_tiles.hpp.
#include "inbatch_tiles.hpp"
#include "refsum.hpp"

namespace {

using namespace inbatch;

constexpr float kNormFloor = 1e-12f;
constexpr uint32_t kTagNoise = 0x58434C31u;   // "XCL1": counter word 3 of the noise stream

// ------------------------------------------------------------------ perturb ------------------------------------------------
template <int LPR>
__global__ __launch_bounds__(256) void perturb_rows_kernel(
    int64_t n_rows, int d4, float4* __restrict__ x, int64_t ldx4, const int64_t* __restrict__ row_ids, float eps,
    uint32_t layer, uint32_t k0, uint32_t k1, const float4* addend, int64_t lda4, float4* S, int64_t lds4, float scale) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t row = t / LPR;
    const int e = (int)(t % LPR);
    const bool live = row < n_rows && e < d4;
    float4 y = mi_f4_zero(), u = mi_f4_zero();
    if (live) {
        y = x[row * ldx4 + e];
        const int64_t id = row_ids ? row_ids[row] : row;
        const MiPhilox w = mi_philox4x32((uint32_t)id, (uint32_t)e, layer, kTagNoise, k0, k1);
        const float s24 = 1.0f / 16777216.0f;
        u = make_float4((float)(w.c[0] >> 8) * s24, (float)(w.c[1] >> 8) * s24, (float)(w.c[2] >> 8) * s24,
                        (float)(w.c[3] >> 8) * s24);
    }
    float ss = fmaf(u.x, u.x, fmaf(u.y, u.y, fmaf(u.z, u.z, u.w * u.w)));
#pragma unroll
    for (int off = LPR / 2; off > 0; off >>= 1) ss += __shfl_xor(ss, off, MI_WAVE);   // LPR divides 64: inside the sub-group
    if (!live) return;
    const float f = eps / fmaxf(sqrtf(ss), kNormFloor);
    auto sgn = [](float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); };
    y.x = fmaf(f * sgn(y.x), u.x, y.x);
    y.y = fmaf(f * sgn(y.y), u.y, y.y);
    y.z = fmaf(f * sgn(y.z), u.z, y.z);
    y.w = fmaf(f * sgn(y.w), u.w, y.w);
    x[row * ldx4 + e] = y;
    if (S) {
        const float4 a = addend ? addend[row * lda4 + e] : mi_f4_zero();
        S[row * lds4 + e] = make_float4((a.x + y.x) * scale, (a.y + y.y) * scale, (a.z + y.z) * scale, (a.w + y.w) * scale);
    }
}

// ------------------------------------------------------------------ contrast: 1. normalise ---------------------------------
// one wavefront per slot, float4 lanes (d <= 256: one float4 per lane)
__global__ __launch_bounds__(256) void contrast_normalise_kernel(
    int64_t batch, int d4, const int64_t* __restrict__ ids, const float4* __restrict__ a, int64_t lda4,
    const float4* __restrict__ b, int64_t ldb4, float inv_tau, float4* __restrict__ u_img, float4* __restrict__ v_img,
    int32_t* __restrict__ id32, float* __restrict__ lq, float* __restrict__ na, float* __restrict__ nb,
    uint32_t* __restrict__ keys, uint32_t* __restrict__ refs) {
    const int64_t s = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / MI_WAVE;
    if (s >= batch) return;
    const int lane = mi_lane();
    const int64_t id = ids[s];
    const bool in = lane < d4;
    const float4 fa = in ? a[id * lda4 + lane] : mi_f4_zero();
    const float4 fb = in ? b[id * ldb4 + lane] : mi_f4_zero();
    const float ra = sqrtf(mi_wave_sum(fmaf(fa.x, fa.x, fmaf(fa.y, fa.y, fmaf(fa.z, fa.z, fa.w * fa.w)))));
    const float rb = sqrtf(mi_wave_sum(fmaf(fb.x, fb.x, fmaf(fb.y, fb.y, fmaf(fb.z, fb.z, fb.w * fb.w)))));
    const float da = fmaxf(ra, kNormFloor), db = fmaxf(rb, kNormFloor);
    if (in) {
        u_img[s * d4 + lane] = make_float4(fa.x / da * inv_tau, fa.y / da * inv_tau, fa.z / da * inv_tau, fa.w / da * inv_tau);
        v_img[s * d4 + lane] = make_float4(fb.x / db, fb.y / db, fb.z / db, fb.w / db);
    }
    if (lane == 0) {
        id32[s] = (int32_t)id;
        lq[s] = 0.f;
        // a norm below the floor: the row is divided by the constant floor, whose derivative does not see the row
        na[s] = ra < kNormFloor ? -da : da;
        nb[s] = rb < kNormFloor ? -db : db;
        if (keys) {
            keys[s] = (uint32_t)id;
            refs[s] = (uint32_t)s;
        }
    }
}

// ------------------------------------------------------------------ contrast: 4. through the normalisation -----------------
// Row r of g_slot holds dL/du_img[r] (r < B) or dL/dv_img[r - B]; in place it becomes scale * dL/d(table row):
//   u side: u = f / |f| / tau   ->  (g / tau - u <u, g> tau) / |f|        v side: v = f / |f|  ->  (g - v <v, g>) / |f|
__global__ __launch_bounds__(256) void contrast_norm_bwd_kernel(
    int64_t batch, int d4, const float4* __restrict__ u_img, const float4* __restrict__ v_img, const float* __restrict__ na,
    const float* __restrict__ nb, float inv_tau, float scale_a, float scale_b, float4* __restrict__ g_slot) {
    const int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / MI_WAVE;
    if (r >= 2 * batch) return;
    const int lane = mi_lane();
    const bool side_b = r >= batch, in = lane < d4;
    const int64_t s = side_b ? r - batch : r;
    const float4 img = in ? (side_b ? v_img : u_img)[s * d4 + lane] : mi_f4_zero();
    const float4 g = in ? g_slot[r * d4 + lane] : mi_f4_zero();
    const float dot = mi_wave_sum(fmaf(img.x, g.x, fmaf(img.y, g.y, fmaf(img.z, g.z, img.w * g.w))));
    const float n = side_b ? nb[s] : na[s];
    const float gin = side_b ? 1.f : inv_tau;                          // d img / d p
    const float back = n < 0.f ? 0.f : (side_b ? dot : dot / inv_tau); // <p, dL/dp> / gin; 0 under the floor
    const float w = (side_b ? scale_b : scale_a) / fabsf(n);
    if (in)
        g_slot[r * d4 + lane] = make_float4(w * (gin * g.x - img.x * back), w * (gin * g.y - img.y * back),
                                            w * (gin * g.z - img.z * back), w * (gin * g.w - img.w * back));
}

// ------------------------------------------------------------------ contrast: 5. slot rows -> table rows -------------------
template <int VPT>
__global__ __launch_bounds__(refsum::kBlock) void contrast_chunk_kernel(int64_t batch, const float* __restrict__ g_side,
                                                                        const uint32_t* __restrict__ keys,
                                                                        const uint32_t* __restrict__ refs, refsum::Dest to) {
    const refsum::Chunk c = refsum::open_chunk(keys, batch);
    if (c.n_here == 0) return;
    refsum::SlotRow term;
    if (c.lane < c.n_here) term.src = refs[c.j0 + c.lane];
    refsum::walk_references<VPT>(c, term, g_side, to.d, to);
}

// ------------------------------------------------------------------ host ---------------------------------------------------
struct ContrastWs {
    float *u_img, *v_img, *g_slot, *lq, *lse, *term, *na, *nb;
    int32_t* id32;
    refsum::Buffers sum;
    bool ok() const { return u_img && v_img && g_slot && lq && lse && term && na && nb && id32 && sum.ok(); }
};

ContrastWs contrast_carve(MiArena& a, int64_t batch, int64_t d) {
    const size_t b = (size_t)batch, bp = (size_t)mi_ceil_div(batch, kTile) * kTile;   // id and statistic arrays: whole tiles
    ContrastWs w;
    w.u_img = a.take<float>(b * d);
    w.v_img = a.take<float>(b * d);
    w.g_slot = a.take<float>(2 * b * d);
    w.id32 = a.take<int32_t>(bp);
    w.lq = a.take<float>(bp);
    w.lse = a.take<float>(bp);
    w.term = a.take<float>(bp);
    w.na = a.take<float>(bp);
    w.nb = a.take<float>(bp);
    w.sum = refsum::take(a, batch, d);
    return w;
}

}  // namespace

extern "C" {

int mi_perturb_rows_f32(int64_t n_rows, int64_t d, float* x, int64_t ldx, const int64_t* row_ids, float eps, int32_t layer,
                        uint64_t seed, uint64_t step, const float* addend, int64_t lda, float* S, int64_t lds, float scale,
                        mi_stream_t stream) {
    MI_CHECK_ARG(n_rows >= 0 && d > 0);
    if (d % 4 != 0 || d > kMaxD) return MI_ERR_UNSUPPORTED;
    MI_CHECK_ARG(layer >= 0 && eps >= 0.f);
    if (n_rows * 64 >= ((int64_t)1 << 40)) return MI_ERR_TOO_LARGE;
    if (n_rows == 0) return 0;
    MI_CHECK_ARG(x && ldx >= d && ldx % 4 == 0 && mi_aligned16(x));
    MI_CHECK_ARG(!addend || S);                                   // an addend has nowhere to go without S
    MI_CHECK_ARG(!S || (lds >= d && lds % 4 == 0 && mi_aligned16(S) && S != x));
    MI_CHECK_ARG(!addend || (lda >= d && lda % 4 == 0 && mi_aligned16(addend) && addend != x));
    MI_CHECK_ARG(!addend || addend != S || lda == lds);           // S may alias addend, row for row
    MI_CHECK_ARG((uintptr_t)row_ids % 8 == 0);
    const uint64_t key = seed + 0x9E3779B97F4A7C15ull * step;
    const uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
    const int d4 = (int)(d / 4);
    int lpr = 1;
    while (lpr < d4) lpr *= 2;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)mi_ceil_div(n_rows * lpr, 256)), block(256);
#define MI_PERTURB(L)                                                                                                         \
    case L:                                                                                                                   \
        hipLaunchKernelGGL(perturb_rows_kernel<L>, grid, block, 0, s, n_rows, d4, reinterpret_cast<float4*>(x), ldx / 4,       \
                           row_ids, eps, (uint32_t)layer, k0, k1, reinterpret_cast<const float4*>(addend), lda / 4,           \
                           reinterpret_cast<float4*>(S), lds / 4, scale);                                                    \
        break;
    switch (lpr) {
        MI_PERTURB(1) MI_PERTURB(2) MI_PERTURB(4) MI_PERTURB(8) MI_PERTURB(16) MI_PERTURB(32) MI_PERTURB(64)
    }
#undef MI_PERTURB
    return mi_launch_status();
}

size_t mi_contrastive_workspace_bytes(int64_t batch, int64_t d, int32_t group) {
    if (!args_in_range(batch, d, group)) return 0;
    const size_t b = (size_t)batch, bp = (size_t)mi_ceil_div(batch, kTile) * kTile;
    return 2 * mi_align_up(b * d * sizeof(float), 256) + mi_align_up(2 * b * d * sizeof(float), 256) +
           6 * mi_align_up(bp * sizeof(float), 256) + refsum::workspace_bytes(batch, d);
}

int mi_contrastive_fwd_bwd_f32(int64_t batch, int32_t group, int64_t d, const int64_t* ids, const float* a, int64_t lda,
                               const float* b, int64_t ldb, float inv_tau, float* loss_out, float* g_a, int64_t ldga,
                               float g_scale_a, float* g_b, int64_t ldgb, float g_scale_b, void* ws, size_t ws_bytes,
                               mi_stream_t stream) {
    MI_CHECK_ARG(batch >= 1 && d > 0);
    if (d % 4 != 0 || d > kMaxD) return MI_ERR_UNSUPPORTED;
    MI_CHECK_ARG(group >= kMinGroup && group <= kMaxGroup && group % kTile == 0);
    MI_CHECK_ARG(inv_tau > 0.f && inv_tau < INFINITY);
    if ((g_a == nullptr) != (g_b == nullptr)) return MI_ERR_UNSUPPORTED;   // both gradients, or the loss-only form
    if (2 * batch >= INT32_MAX) return MI_ERR_TOO_LARGE;
    MI_CHECK_ARG(ids && a && b && loss_out && ws);
    MI_CHECK_ARG(lda >= d && ldb >= d && lda % 4 == 0 && ldb % 4 == 0 && (!g_a || (ldga >= d && ldgb >= d)));
    MI_CHECK_ARG(mi_aligned16(a) && mi_aligned16(b) && mi_aligned16(ws) && (uintptr_t)ids % 8 == 0);
    MI_CHECK_ARG(((uintptr_t)loss_out | (uintptr_t)g_a | (uintptr_t)g_b) % 4 == 0);
    if (ws_bytes < mi_contrastive_workspace_bytes(batch, d, group)) return MI_ERR_WORKSPACE;
    MiArena arena(ws, ws_bytes);
    const ContrastWs w = contrast_carve(arena, batch, d);
    if (!w.ok()) return MI_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int64_t n_tiles = mi_ceil_div(batch, kTile);
    const int d4 = (int)(d / 4), nq = (int)mi_align_up((size_t)(d4 + 1) / 2, kLoadGroup);   // k steps: whole groups
    const size_t lds = (size_t)kTile * (2 * nq + 1) * sizeof(float4);
    refsum::Sort sorted;
    if (g_a) {
        const int rc = refsum::plan_sort(w.sum, batch, false, s, sorted);
        if (rc) return rc;
    }
    // ---- nothing has been enqueued up to here ----
    const float4* u_img = reinterpret_cast<const float4*>(w.u_img);
    const float4* v_img = reinterpret_cast<const float4*>(w.v_img);
    hipLaunchKernelGGL(contrast_normalise_kernel, dim3((unsigned)mi_ceil_div(batch * MI_WAVE, 256)), dim3(256), 0, s, batch,
                       d4, ids, reinterpret_cast<const float4*>(a), lda / 4, reinterpret_cast<const float4*>(b), ldb / 4,
                       inv_tau, reinterpret_cast<float4*>(w.u_img), reinterpret_cast<float4*>(w.v_img), w.id32, w.lq, w.na,
                       w.nb, g_a ? w.sum.k0 : nullptr, g_a ? w.sum.r0 : nullptr);
    hipLaunchKernelGGL(inbatch_stats_kernel, dim3((unsigned)n_tiles), dim3(MI_WAVE), lds, s, batch, (int)group, d4, nq, u_img,
                       v_img, (const int32_t*)w.id32, (const int32_t*)w.id32, (const float*)w.lq, w.lse, w.term);
    if (g_a) {
        refsum::with_vpt(mi_ceil_div(d, 32), [&](auto nt) {
            constexpr int NT = decltype(nt)::value;
            hipLaunchKernelGGL(inbatch_sweep_kernel<NT>, dim3((unsigned)n_tiles, 2), dim3(MI_WAVE), lds, s, batch, (int)group,
                               (int)d, nq, u_img, v_img, (const int32_t*)w.id32, (const int32_t*)w.id32, (const float*)w.lq,
                               (const float*)w.lse, 1.0f / (float)batch, w.g_slot);
        });
        hipLaunchKernelGGL(contrast_norm_bwd_kernel, dim3((unsigned)mi_ceil_div(2 * batch * MI_WAVE, 256)), dim3(256), 0, s,
                           batch, d4, u_img, v_img, (const float*)w.na, (const float*)w.nb, inv_tau, g_scale_a, g_scale_b,
                           reinterpret_cast<float4*>(w.g_slot));
        const int rc = refsum::sort(w.sum, batch, s, sorted);
        if (rc) return rc;
        for (int side = 0; side < 2; ++side) {   // the partial rows are reused: the launches of a stream run in order
            const refsum::Dest to{side ? g_b : g_a, side ? ldgb : ldga, w.sum.part_head, w.sum.part_tail, (int)d, true};
            const float* g_side = w.g_slot + (side ? batch * d : 0);
            refsum::with_vpt(mi_ceil_div(d, MI_WAVE), [&](auto vpt) {
                constexpr int V = decltype(vpt)::value < 4 ? decltype(vpt)::value : 4;   // d <= 256
                hipLaunchKernelGGL(contrast_chunk_kernel<V>, refsum::chunk_grid(batch), dim3(refsum::kBlock), 0, s, batch,
                                   g_side, (const uint32_t*)sorted.keys.current(), (const uint32_t*)sorted.refs.current(), to);
                refsum::launch_combine<V>(sorted, batch, to, s);
            });
        }
    }
    refsum::launch_finish(batch, w.term, w.lq, 1.0f / (float)batch, 0.f, loss_out, s);
    return mi_launch_status();
}

}  // extern "C"
