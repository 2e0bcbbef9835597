// N5 evaluation: the representation of EVERY item in one call (include/laplace_hip.h, mi_pinsage_embed_items_f32).
//
// The reference embeds the catalogue batch by batch (pinsage/model.py:120-134 over collate_test, pinsage/sampler.py:181-185):
// sample_blocks around 32 item ids, get_repr over the blocks, 3 299 batches at H&M's 105 542 items.  A walk's draws are keyed
// on (walk, traversal, sampler layer, start item, seed, step) and eval blocks carry no label pairs, so for one (seed, step)
// an item's top-T neighbours at a sampler layer are the same in every batch: the batched get_repr equals a layer-by-layer
// pass over the whole catalogue, each item's neighbours sampled once per layer and each dense layer run once per item.
//
//   h_0 = proj[0 .. n_items)
//   for model layer m (sampler layer NL - 1 - m: sample_blocks builds layer 0 around the seeds, the model consumes the
//   blocks in reverse):
//     nb, w   = top-T neighbours of every item                                  neighbors_kernel, seed list = identity
//     n       = relu(Q_m h_m + b_Q)                                             pin_embed_q_kernel
//     h_{m+1} = l2norm(relu(W_m [sum_j w_j n[nb_j] / max(sum_j w_j, 1), h_m] + b_W))   pin_embed_layer_kernel
//   out = proj + h_NL                                                           (the last layer's epilogue)
//
// The results differ from the batched path only in the order of at most T terms of the weighted mean (block-local numbering
// sorts a block's CSR columns differently): equal to rounding, not bitwise.  Deterministic, no atomics.
//
// Both row kernels hold a row of `hidden` floats in hidden / 4 lanes (lane c: columns 4c .. 4c + 3; groups padded to a power
// of two), 64 / gp rows per wavefront — 16 at the reference's hidden 16, a 64-byte row.  The weights sit transposed in LDS
// (W^T[k][o], float4 per lane and k); a row's inputs reach the other lanes of its group by shuffles, so every output is one
// k-ascending fma chain plus the bias, as on the GEMM kernel.
#include "common.hpp"

bool pinsage_neighbors_all(int64_t n_items, const int32_t* iu_ptr, const int32_t* iu_idx, const int32_t* ui_ptr,
                           const int32_t* ui_idx, int walk_length, double restart_prob, int num_walks, int T, int layer,
                           uint64_t seed, uint64_t step, int64_t* nb, int64_t* wt, hipStream_t stream);   // csrc/pinsage.hip

namespace {

constexpr int kEmbBlock = 256;
constexpr int kEmbMaxT = 16;

__device__ __forceinline__ float4 shfl4(const float4& v, int src) {
    return make_float4(__shfl(v.x, src, MI_WAVE), __shfl(v.y, src, MI_WAVE), __shfl(v.z, src, MI_WAVE), __shfl(v.w, src, MI_WAVE));
}

__device__ __forceinline__ float4 relu4(const float4& v) {
    return make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f));
}

// acc += W^T[k0 + 4j + q][4c .. 4c + 3] * x_{4j + q} for j = 0 .. G-1, q = 0 .. 3 (k ascending); x is spread over the row's group:
// lane base + j holds x_{4j .. 4j + 3}.  wt points at W^T row k0 (float4 units, h4 per row).  Every lane of the wavefront runs
// it (shuffles); lanes without a row pass zeros and a valid c.
__device__ __forceinline__ void group_matvec(float4& acc, const float4* wt, int h4, int c, const float4& x, int base, int G) {
    for (int j = 0; j < G; ++j) {
        const float4 xj = shfl4(x, base + j);
        const float4* w = wt + (4 * j) * h4 + c;
        mi_f4_fma(acc, xj.x, w[0]);
        mi_f4_fma(acc, xj.y, w[h4]);
        mi_f4_fma(acc, xj.z, w[2 * h4]);
        mi_f4_fma(acc, xj.w, w[3 * h4]);
    }
}

// W [H, K] (nn.Linear layout) -> LDS W^T [K][H]
__device__ __forceinline__ void stage_transposed(float* lds, const float* __restrict__ w, int H, int K) {
    for (int i = threadIdx.x; i < H * K; i += kEmbBlock) {
        const int k = i / H, o = i - k * H;
        lds[i] = w[(int64_t)o * K + k];
    }
    __syncthreads();
}

// n = relu(Q h + b) over all rows
__global__ __launch_bounds__(kEmbBlock) void pin_embed_q_kernel(int64_t n, int H, int gp, const float4* __restrict__ h,
                                                                const float* __restrict__ qw, const float4* __restrict__ qb,
                                                                float4* __restrict__ out) {
    extern __shared__ float4 lds4[];
    stage_transposed(reinterpret_cast<float*>(lds4), qw, H, H);
    const int h4 = H / 4;
    const int lane = mi_lane(), c = lane & (gp - 1), base = lane - c;
    const int64_t r = (int64_t)blockIdx.x * (kEmbBlock / gp) + threadIdx.x / gp;
    const bool act = r < n && c < h4;
    const int cc = c < h4 ? c : 0;
    const float4 x = act ? h[r * h4 + c] : mi_f4_zero();
    float4 acc = mi_f4_zero();
    group_matvec(acc, lds4, h4, cc, x, base, h4);
    if (act) out[r * h4 + c] = relu4(mi_f4_add(acc, qb[c]));
}

// One WeightedSAGEConv over a fixed neighbour table (pinsage/layers.py:121-156 in eval mode), fused:
//   agg = sum_j (w_j / max(sum w, 1)) n[nb_j]  (j ascending, -1 entries skipped; no neighbour: agg = 0)
//   z = relu(W [agg, h] + b),  out = z / (||z|| or 1)  (+ proj, the last layer's h_dst_final + h)
__global__ __launch_bounds__(kEmbBlock) void pin_embed_layer_kernel(int64_t n, int H, int gp, int T, const int64_t* __restrict__ nb,
                                                                    const int64_t* __restrict__ cnt, const float4* __restrict__ nrow,
                                                                    const float4* __restrict__ h, const float* __restrict__ ww,
                                                                    const float4* __restrict__ wb, const float4* __restrict__ proj,
                                                                    float4* __restrict__ out) {
    extern __shared__ float4 lds4[];
    stage_transposed(reinterpret_cast<float*>(lds4), ww, H, 2 * H);
    const int h4 = H / 4;
    const int lane = mi_lane(), c = lane & (gp - 1), base = lane - c;
    const int64_t r = (int64_t)blockIdx.x * (kEmbBlock / gp) + threadIdx.x / gp;
    const bool act = r < n && c < h4;
    const int cc = c < h4 ? c : 0;
    float4 agg = mi_f4_zero();
    float4 x = mi_f4_zero();
    if (act) {
        int64_t v[kEmbMaxT];
        float w[kEmbMaxT];
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < kEmbMaxT; ++j) {
            v[j] = -1;
            w[j] = 0.f;
            if (j < T) {
                v[j] = nb[r * T + j];
                w[j] = (float)cnt[r * T + j];
                if (v[j] >= 0) sum += w[j];
            }
        }
        const float den = fmaxf(sum, 1.0f);
#pragma unroll
        for (int j = 0; j < kEmbMaxT; ++j)
            if (v[j] >= 0) mi_f4_fma(agg, w[j] / den, nrow[v[j] * h4 + c]);
        x = h[r * h4 + c];
    }
    float4 acc = mi_f4_zero();
    group_matvec(acc, lds4, h4, cc, agg, base, h4);             // k in [0, H): the neighbourhood mean
    group_matvec(acc, lds4 + H * h4, h4, cc, x, base, h4);      // k in [H, 2H): the row itself
    float4 z = act ? relu4(mi_f4_add(acc, wb[cc])) : mi_f4_zero();
    float ss = z.x * z.x + z.y * z.y + z.z * z.z + z.w * z.w;
    for (int off = gp >> 1; off > 0; off >>= 1) ss += __shfl_xor(ss, off, MI_WAVE);   // fixed butterfly within the group
    const float nrm = sqrtf(ss);
    const float d = nrm == 0.f ? 1.f : nrm;
    if (!act) return;
    z = make_float4(z.x / d, z.y / d, z.z / d, z.w / d);
    if (proj) z = mi_f4_add(z, proj[r * h4 + c]);
    out[r * h4 + c] = z;
}

bool set_lds_limit(const void* fn, size_t bytes, bool* done) {
    if (bytes <= 64 * 1024 || *done) return true;
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) return false;
    *done = true;
    return true;
}

}  // namespace

extern "C" size_t mi_pinsage_embed_items_workspace_bytes(int64_t n_items, int32_t hidden, int32_t num_neighbors) {
    if (n_items <= 0 || hidden <= 0 || num_neighbors <= 0) return 256;
    return 2 * mi_align_up((size_t)n_items * (size_t)num_neighbors * sizeof(int64_t), 256) +   // neighbour table, visit counts
           3 * mi_align_up((size_t)n_items * (size_t)hidden * sizeof(float), 256);             // n, two layer outputs
}

extern "C" int mi_pinsage_embed_items_f32(const mi_pinsage_model* model, const int32_t* iu_ptr, const int32_t* iu_idx,
                                          const int32_t* ui_ptr, const int32_t* ui_idx, int32_t walk_length, double restart_prob,
                                          int32_t num_walks, int32_t num_neighbors, uint64_t seed, uint64_t step, float* out,
                                          void* ws, size_t ws_bytes, mi_stream_t stream) {
    MI_CHECK_ARG(model && iu_ptr && iu_idx && ui_ptr && ui_idx && out && ws);
    MI_CHECK_ARG(walk_length > 0 && num_walks > 0 && num_neighbors > 0 && restart_prob >= 0.0 && restart_prob < 1.0);
    const mi_pinsage_model& M = *model;
    const int NL = M.n_layers, H = M.hidden, T = num_neighbors;
    const int64_t n = M.n_items;
    if (NL < 1 || NL > MI_PINSAGE_MAX_LAYERS || H < 4 || H % 4 != 0 || H > 128 || T > kEmbMaxT) return MI_ERR_UNSUPPORTED;
    MI_CHECK_ARG(n > 0 && M.proj);
    if (n >= INT32_MAX) return MI_ERR_TOO_LARGE;
    if (!mi_aligned16(M.proj) || !mi_aligned16(out)) return MI_ERR_UNSUPPORTED;
    for (int l = 0; l < NL; ++l) {
        const mi_pinsage_conv& cv = M.conv[l];
        MI_CHECK_ARG(cv.q_w && cv.q_b && cv.w_w && cv.w_b);
        if (!mi_aligned16(cv.q_b) || !mi_aligned16(cv.w_b)) return MI_ERR_UNSUPPORTED;
    }
    if (ws_bytes < mi_pinsage_embed_items_workspace_bytes(n, H, T)) return MI_ERR_WORKSPACE;
    const size_t lds_q = (size_t)H * H * sizeof(float), lds_w = (size_t)2 * H * H * sizeof(float);
    static bool q_attr = false, w_attr = false;
    if (!set_lds_limit(reinterpret_cast<const void*>(pin_embed_q_kernel), lds_q, &q_attr) ||
        !set_lds_limit(reinterpret_cast<const void*>(pin_embed_layer_kernel), lds_w, &w_attr))
        return MI_ERR_UNSUPPORTED;
    MiArena ar(ws, ws_bytes);
    int64_t* nb = ar.take<int64_t>((size_t)n * T);
    int64_t* cnt = ar.take<int64_t>((size_t)n * T);
    float* nbuf = ar.take<float>((size_t)n * H);
    float* hbuf[2] = {ar.take<float>((size_t)n * H), ar.take<float>((size_t)n * H)};
    if (!nb || !cnt || !nbuf || !hbuf[0] || !hbuf[1]) return MI_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    int gp = 1;
    while (gp < H / 4) gp <<= 1;
    const unsigned grid = (unsigned)mi_ceil_div(n, kEmbBlock / gp);
    const float* h = M.proj;   // h_0: the projector rows of the items (the table's last row is the padding id's)
    for (int m = 0; m < NL; ++m) {
        const mi_pinsage_conv& cv = M.conv[m];
        if (!pinsage_neighbors_all(n, iu_ptr, iu_idx, ui_ptr, ui_idx, walk_length, restart_prob, num_walks, T, NL - 1 - m, seed,
                                   step, nb, cnt, s))
            return MI_ERR_UNSUPPORTED;   // only the first layer can get here: nothing enqueued
        hipLaunchKernelGGL(pin_embed_q_kernel, dim3(grid), dim3(kEmbBlock), lds_q, s, n, H, gp, reinterpret_cast<const float4*>(h),
                           cv.q_w, reinterpret_cast<const float4*>(cv.q_b), reinterpret_cast<float4*>(nbuf));
        const bool last = m == NL - 1;
        float* dst = last ? out : hbuf[m & 1];
        hipLaunchKernelGGL(pin_embed_layer_kernel, dim3(grid), dim3(kEmbBlock), lds_w, s, n, H, gp, T, nb, cnt,
                           reinterpret_cast<const float4*>(nbuf), reinterpret_cast<const float4*>(h), cv.w_w,
                           reinterpret_cast<const float4*>(cv.w_b), last ? reinterpret_cast<const float4*>(M.proj) : nullptr,
                           reinterpret_cast<float4*>(dst));
        const int rc = mi_launch_status();
        if (rc) return rc;
        h = dst;
    }
    return 0;
}
