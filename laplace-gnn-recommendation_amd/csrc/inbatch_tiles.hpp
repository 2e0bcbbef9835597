// The two group kernels of the in-batch softmax, shared by inbatch.hip and contrastive.hip: the row statistics and the gradient
// sweeps over the G x G scores of a group of G slots.  The caller provides two contiguous [B, d] row images (u_img: the
// slots' own rows; v_img: the candidates'), the slots' two mask ids as int32 and a per-candidate logit offset lq, all padded
// to whole tiles of 32 slots.  This file owns the group window, the masks and the logit offset; the score tiles, their lane
// map and k order, the running (max, sum) and the gradient product are those of loss_tiles.hpp.
#pragma once
#include "loss_tiles.hpp"

namespace inbatch {

using namespace loss_tiles;

constexpr int kMinGroup = 32, kMaxGroup = 4096;
// A k step's A chunk is loaded where it is used.  Groups of 4 (fullsoftmax.hip) give the same bits and 4 % faster calls at
// d = 128, but their registers cost inbatch_sweep_kernel<1> a wave per SIMD (profiles/loss_tiles.md).
constexpr int kLoadGroup = 1;

inline bool args_in_range(int64_t batch, int64_t d, int32_t group) {
    return batch >= 1 && 2 * batch < INT32_MAX && d >= 4 && d % 4 == 0 && d <= kMaxD && group >= kMinGroup &&
           group <= kMaxGroup && group % kTile == 0;
}

// ------------------------------------------------------------------ 2. row statistics --------------------------------------
// One wavefront per 32 user slots: their (max, sum) over the candidate tiles of the group, tiles ascending -> lse[b] and the
// slot's loss term.
static __global__ __launch_bounds__(MI_WAVE) void inbatch_stats_kernel(
    int64_t batch, int group, int d4, int nq, const float4* __restrict__ u_img, const float4* __restrict__ v_img,
    const int32_t* __restrict__ uid, const int32_t* __restrict__ pid, const float* __restrict__ lq,
    float* __restrict__ lse_out, float* __restrict__ term_out) {
    extern __shared__ float4 tile[];
    const int lane = mi_lane(), c = lane & 31, h = lane >> 5;
    const Rows users{u_img, d4, batch}, cands{v_img, d4, batch};
    const int64_t b0 = (int64_t)blockIdx.x * kTile;
    const int64_t g0 = b0 / group * group, g1 = min(g0 + group, batch);
    load_owned_tile(tile, users, b0, d4, nq);
    __syncthreads();
    const int64_t b = b0 + c;
    const int64_t bb = min(b, batch - 1);
    const int32_t my_u = uid[bb], my_p = pid[bb];
    const float ninf = -INFINITY;
    MaxSum run;
    float diag = ninf;
    for (int64_t j0 = g0; j0 < g1; j0 += kTile) {
        const f32x16 acc = score_tile<kLoadGroup>(cands, j0, d4, nq, tile);
        float x[16];
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {   // the arrays are padded to whole tiles: these reads stay inside them
            const int64_t base = j0 + 8 * q4 + 4 * h;
            const int4 pj = *reinterpret_cast<const int4*>(pid + base);
            const int4 uj = *reinterpret_cast<const int4*>(uid + base);
            const float4 lj = *reinterpret_cast<const float4*>(lq + base);
            const int32_t pjs[4] = {pj.x, pj.y, pj.z, pj.w}, ujs[4] = {uj.x, uj.y, uj.z, uj.w};
            const float ljs[4] = {lj.x, lj.y, lj.z, lj.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int64_t j = base + i;
                const float l = acc[4 * q4 + i] - ljs[i];
                const bool out = j >= batch || (j != b && (pjs[i] == my_p || ujs[i] == my_u));
                x[4 * q4 + i] = out ? ninf : l;
                if (j == b) diag = l;
            }
        }
        lse_add_tile(run, x);
    }
    const MaxSum all = lse_fold_halves(run, h);
    diag = fmaxf(diag, __shfl_xor(diag, 32, MI_WAVE));
    if (b < batch && h == 0) {   // the slot itself is never masked: the maximum is finite
        const float lse = all.m + logf(all.s);
        lse_out[b] = lse;
        term_out[b] = lse - diag;
    }
}

// ------------------------------------------------------------------ 3. gradient sweeps -------------------------------------
// blockIdx.y = 0: the owned slots are users (dL/df[users_b] = sum_j c[b,j] f[pos_j], streamed rows = positives);
// blockIdx.y = 1: the owned slots are positives (dL/df[pos_j] = sum_b c[b,j] f[users_b], streamed rows = users).
// One wavefront owns its 32 output rows for the whole sweep over the group: one writer per slot row.
template <int NT>
static __global__ __launch_bounds__(MI_WAVE) void inbatch_sweep_kernel(
    int64_t batch, int group, int d, int nq, const float4* __restrict__ u_img, const float4* __restrict__ v_img,
    const int32_t* __restrict__ uid, const int32_t* __restrict__ pid, const float* __restrict__ lq,
    const float* __restrict__ lse, float w /* g_scale / B */, float* __restrict__ g_slot /* [2B, d]: users, positives */) {
    extern __shared__ float4 tile[];
    const int lane = mi_lane(), c = lane & 31, h = lane >> 5;
    const int d4 = d / 4;
    const bool own_user = blockIdx.y == 0;
    const Rows own{own_user ? u_img : v_img, d4, batch}, str{own_user ? v_img : u_img, d4, batch};
    const int64_t o0 = (int64_t)blockIdx.x * kTile;
    const int64_t g0 = o0 / group * group, g1 = min(g0 + group, batch);
    load_owned_tile(tile, own, o0, d4, nq);
    __syncthreads();
    const int64_t o = o0 + c;
    const int64_t oo = min(o, batch - 1);
    const int32_t my_u = uid[oo], my_p = pid[oo];
    const float my_lq = lq[oo], my_lse = lse[oo];
    f32x16 out[NT];
    grad_zero(out);
    for (int64_t r0 = g0; r0 < g1; r0 += kTile) {
        const f32x16 acc = score_tile<kLoadGroup>(str, r0, d4, nq, tile);
        f32x16 cf;
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
            const int64_t base = r0 + 8 * q4 + 4 * h;
            const int4 pr = *reinterpret_cast<const int4*>(pid + base);
            const int4 ur = *reinterpret_cast<const int4*>(uid + base);
            const float4 lr = *reinterpret_cast<const float4*>(lq + base);
            const float4 sr = *reinterpret_cast<const float4*>(lse + base);
            const int32_t prs[4] = {pr.x, pr.y, pr.z, pr.w}, urs[4] = {ur.x, ur.y, ur.z, ur.w};
            const float lrs[4] = {lr.x, lr.y, lr.z, lr.w}, srs[4] = {sr.x, sr.y, sr.z, sr.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int64_t r = base + i;
                // the logit as stats_kernel formed it: score - logq[candidate's item]; then the user's lse
                const float l = acc[4 * q4 + i] - (own_user ? lrs[i] : my_lq);
                const float e = expf(l - (own_user ? my_lse : srs[i]));
                const bool outside = r >= batch || o >= batch || (r != o && (prs[i] == my_p || urs[i] == my_u));
                cf[4 * q4 + i] = outside ? 0.f : w * (e - (r == o ? 1.f : 0.f));
            }
        }
        grad_add_tile(out, cf, str, r0, d);
    }
    grad_store(out, g_slot + (own_user ? 0 : batch * d), d, o0, batch, d);
}

}  // namespace inbatch
