// In-batch sampled softmax for the LightGCN trainer (mi_inbatch_softmax_fwd_bwd_f32; the rule is in the header): the other
// positives of a slot's group of G slots are its negatives.  The G x G scores of a group are 32 x 32 score tiles
// (loss_tiles.hpp: the lane map, the k order and the rescale order that its passes share, so they see the same score bits).
//   1. gather_kernel   the B user rows and B positive rows of final_emb become two contiguous [B, d] images (through
//                      node_map when given); ids as int32, logq[pos_b] and the slot's L2 term beside them
//   2. stats_kernel    one wavefront per 32 user slots: their scores against every 32-candidate tile of the group, masks
//                      and - logq in registers, a running maximum and sum per lane -> lse[b] and the slot's loss term
//   3. sweep_kernel    one wavefront per 32 OWNED slots, twice: the user rows of a tile (dL/df[users_b]) and the positive
//                      rows of a tile (dL/df[pos_j]), the other side's rows streaming past.  One wavefront owns its 32
//                      output rows for the whole sweep: one writer per slot row.
//   4. refs / sort / chunk / combine   the 2B slot rows become rows of g_final: the sorted-reference segmented sum of
//                      refsum.hpp, with a slot row as each reference's only term; reg_w from the run lengths
//   5. refsum::finish_kernel   loss = sum(term) / B + lambda * sum(reg), one block, fixed order
// No float atomics; every order of summation is a function of (B, G, d) and the ids: two calls give equal bits.
// This file owns passes 1 and 4 and the host entry; passes 2 and 3 are in inbatch_tiles.hpp, which contrastive.hip runs too.
#include "inbatch_tiles.hpp"
#include "refsum.hpp"

namespace {

using namespace inbatch;

// ------------------------------------------------------------------ 1. gather ----------------------------------------------
// one wavefront per slot, float4 lanes
__global__ __launch_bounds__(256) void inbatch_gather_kernel(
    int64_t batch, int d4, int64_t n_users, const int64_t* __restrict__ users, const int64_t* __restrict__ pos,
    const float4* __restrict__ fin, int64_t ldf4, const float4* __restrict__ e0, int64_t lde4,
    const int32_t* __restrict__ node_map, const float* __restrict__ logq, float4* __restrict__ u_img,
    float4* __restrict__ v_img, int32_t* __restrict__ uid, int32_t* __restrict__ pid, float* __restrict__ lq,
    float* __restrict__ reg_out) {
    const int64_t b = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / MI_WAVE;
    if (b >= batch) return;
    const int lane = mi_lane();
    const int64_t u = users[b], p = n_users + pos[b];
    const float4* uf = fin + (node_map ? (int64_t)node_map[u] : u) * ldf4;
    const float4* pf = fin + (node_map ? (int64_t)node_map[p] : p) * ldf4;
    const float4* u0 = e0 + u * lde4;
    const float4* p0 = e0 + p * lde4;
    float rg = 0.f;
    for (int e = lane; e < d4; e += MI_WAVE) {
        u_img[b * d4 + e] = uf[e];
        v_img[b * d4 + e] = pf[e];
        rg = add_squares(rg, u0[e], p0[e]);
    }
    rg = mi_wave_sum(rg);
    if (lane == 0) {
        uid[b] = (int32_t)users[b];
        pid[b] = (int32_t)pos[b];
        lq[b] = logq ? logq[pos[b]] : 0.f;
        reg_out[b] = rg;
    }
}

// ------------------------------------------------------------------ 4. slot rows -> node rows ------------------------------
__global__ void inbatch_refs_kernel(int64_t batch, int64_t n_users, const int64_t* __restrict__ users,
                                    const int64_t* __restrict__ pos, const int32_t* __restrict__ node_map,
                                    uint32_t* __restrict__ keys, uint32_t* __restrict__ refs) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // reference id = role * batch + b = its row of g_slot
    if (r >= 2 * batch) return;
    const int64_t node = r < batch ? users[r] : n_users + pos[r - batch];
    keys[r] = (uint32_t)(node_map ? node_map[node] : node);
    refs[r] = (uint32_t)r;
}

template <int VPT>  // floats of a row per lane: ceil(d / 64)
__global__ __launch_bounds__(refsum::kBlock) void inbatch_chunk_kernel(
    int64_t batch, int64_t n_users, const int64_t* __restrict__ users, const int64_t* __restrict__ pos,
    const float* __restrict__ g_slot, const uint32_t* __restrict__ keys, const uint32_t* __restrict__ refs, refsum::Dest to,
    float* __restrict__ reg_w, float reg_unit /* 2 * lambda * reg_scale: one reference's share */) {
    const int64_t n_ref = 2 * batch;
    const refsum::Chunk c = refsum::open_chunk(keys, n_ref);
    if (c.n_here == 0) return;
    refsum::SlotRow term;
    if (c.lane < c.n_here) {
        term.src = refs[c.j0 + c.lane];
        if (reg_w) {
            const int64_t len = refsum::run_length(keys, c.j0 + c.lane, n_ref);
            if (len) reg_w[term.src < batch ? users[term.src] : n_users + pos[term.src - batch]] = (float)len * reg_unit;
        }
    }
    refsum::walk_references<VPT>(c, term, g_slot, to.d, to);
}

// ------------------------------------------------------------------ host ---------------------------------------------------
struct Workspace {
    float *u_img, *v_img, *g_slot, *lq, *lse, *term, *reg;
    int32_t *uid, *pid;
    refsum::Buffers sum;   // partial rows of d floats: this entry knows its d
    bool ok() const { return u_img && v_img && g_slot && lq && lse && term && reg && uid && pid && sum.ok(); }
};

Workspace carve(MiArena& a, int64_t batch, int64_t d) {
    const size_t b = (size_t)batch, bp = (size_t)mi_ceil_div(batch, kTile) * kTile;   // id and statistic arrays: whole tiles
    const size_t n_ref = 2 * b;
    Workspace w;
    w.u_img = a.take<float>(b * d);
    w.v_img = a.take<float>(b * d);
    w.g_slot = a.take<float>(n_ref * d);
    w.uid = a.take<int32_t>(bp);
    w.pid = a.take<int32_t>(bp);
    w.lq = a.take<float>(bp);
    w.lse = a.take<float>(bp);
    w.term = a.take<float>(bp);
    w.reg = a.take<float>(bp);
    w.sum = refsum::take(a, (int64_t)n_ref, d);
    return w;
}

}  // namespace

extern "C" {

size_t mi_inbatch_softmax_workspace_bytes(int64_t batch, int64_t d, int32_t group) {
    if (!args_in_range(batch, d, group)) return 0;
    const size_t b = (size_t)batch, bp = (size_t)mi_ceil_div(batch, kTile) * kTile;
    const size_t n_ref = 2 * b;
    return 2 * mi_align_up(b * d * sizeof(float), 256) + mi_align_up(n_ref * d * sizeof(float), 256) +
           6 * mi_align_up(bp * sizeof(float), 256) + refsum::workspace_bytes((int64_t)n_ref, d);
}

int mi_inbatch_softmax_fwd_bwd_f32(int64_t batch, int32_t group, int64_t d, int64_t n_users, const int64_t* users,
                                   const int64_t* pos, const float* final_emb, int64_t ldf, const float* e0, int64_t lde,
                                   float lambda, float g_scale, float reg_scale, float* loss_out, float* g_final,
                                   int64_t ldg, float* reg_w, const int32_t* node_map, const float* logq, void* ws,
                                   size_t ws_bytes, mi_stream_t stream) {
    MI_CHECK_ARG(batch >= 1 && d > 0 && n_users >= 0);
    if (d % 4 != 0 || d > kMaxD) return MI_ERR_UNSUPPORTED;
    MI_CHECK_ARG(group >= kMinGroup && group <= kMaxGroup && group % kTile == 0);
    if (!g_final && reg_w) return MI_ERR_UNSUPPORTED;   // the loss-only form has no reference list to count the nodes from
    if (2 * batch >= INT32_MAX) return MI_ERR_TOO_LARGE;
    MI_CHECK_ARG(users && pos && final_emb && e0 && loss_out && ws);
    MI_CHECK_ARG(ldf >= d && lde >= d && ldf % 4 == 0 && lde % 4 == 0 && (!g_final || ldg >= d));
    MI_CHECK_ARG(mi_aligned16(final_emb) && mi_aligned16(e0) && mi_aligned16(ws));
    MI_CHECK_ARG(((uintptr_t)users | (uintptr_t)pos) % 8 == 0);
    MI_CHECK_ARG(((uintptr_t)loss_out | (uintptr_t)g_final | (uintptr_t)reg_w | (uintptr_t)node_map | (uintptr_t)logq) % 4 == 0);
    if (ws_bytes < mi_inbatch_softmax_workspace_bytes(batch, d, group)) return MI_ERR_WORKSPACE;
    MiArena arena(ws, ws_bytes);
    const Workspace w = carve(arena, batch, d);
    if (!w.ok()) return MI_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int64_t n_ref = 2 * batch, n_tiles = mi_ceil_div(batch, kTile);
    const int d4 = (int)(d / 4), nq = (int)mi_align_up((size_t)(d4 + 1) / 2, kLoadGroup);   // k steps: whole groups
    const size_t lds = (size_t)kTile * (2 * nq + 1) * sizeof(float4);   // 33 280 bytes at d = 256
    refsum::Sort sorted;
    if (g_final) {
        const int rc = refsum::plan_sort(w.sum, n_ref, node_map != nullptr, s, sorted);
        if (rc) return rc;
    }
    // ---- nothing has been enqueued up to here ----
    const float4* u_img = reinterpret_cast<const float4*>(w.u_img);
    const float4* v_img = reinterpret_cast<const float4*>(w.v_img);
    hipLaunchKernelGGL(inbatch_gather_kernel, dim3((unsigned)mi_ceil_div(batch * MI_WAVE, 256)), dim3(256), 0, s, batch, d4,
                       n_users, users, pos, reinterpret_cast<const float4*>(final_emb), ldf / 4,
                       reinterpret_cast<const float4*>(e0), lde / 4, node_map, logq, reinterpret_cast<float4*>(w.u_img),
                       reinterpret_cast<float4*>(w.v_img), w.uid, w.pid, w.lq, w.reg);
    hipLaunchKernelGGL(inbatch_stats_kernel, dim3((unsigned)n_tiles), dim3(MI_WAVE), lds, s, batch, (int)group, d4, nq, u_img,
                       v_img, w.uid, w.pid, w.lq, w.lse, w.term);
    if (g_final) {
        const float wgt = g_scale / (float)batch;
        refsum::with_vpt(mi_ceil_div(d, 32), [&](auto nt) {
            constexpr int NT = decltype(nt)::value;
            hipLaunchKernelGGL(inbatch_sweep_kernel<NT>, dim3((unsigned)n_tiles, 2), dim3(MI_WAVE), lds, s, batch, (int)group,
                               (int)d, nq, u_img, v_img, w.uid, w.pid, w.lq, w.lse, wgt, w.g_slot);
        });
        hipLaunchKernelGGL(inbatch_refs_kernel, dim3((unsigned)mi_ceil_div(n_ref, 256)), dim3(256), 0, s, batch, n_users, users,
                           pos, node_map, w.sum.k0, w.sum.r0);
        const int rc = refsum::sort(w.sum, n_ref, s, sorted);
        if (rc) return rc;
        const refsum::Dest to{g_final, ldg, w.sum.part_head, w.sum.part_tail, (int)d};
        refsum::with_vpt(mi_ceil_div(d, MI_WAVE), [&](auto vpt) {
            constexpr int V = decltype(vpt)::value < 4 ? decltype(vpt)::value : 4;   // d <= 256
            hipLaunchKernelGGL(inbatch_chunk_kernel<V>, refsum::chunk_grid(n_ref), dim3(refsum::kBlock), 0, s, batch, n_users,
                               users, pos, (const float*)w.g_slot, (const uint32_t*)sorted.keys.current(),
                               (const uint32_t*)sorted.refs.current(), to, reg_w, 2.0f * reg_scale * lambda);
            refsum::launch_combine<V>(sorted, n_ref, to, s);
        });
    }
    refsum::launch_finish(batch, w.term, w.reg, 1.0f / (float)batch, lambda, loss_out, s);
    return mi_launch_status();
}

}  // extern "C"
