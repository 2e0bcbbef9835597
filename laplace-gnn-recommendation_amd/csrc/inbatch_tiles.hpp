// The in-batch softmax's score tiles, shared by inbatch.hip and contrastive.hip: the G x G scores of a group of G slots are
// products of 32 x 32 tiles on the exact-f32 matrix instruction (v_mfma_f32_32x32x2_f32: bit for bit a k-ordered fmaf chain)
// and never leave the registers; every pass that needs them computes them again.  The caller provides two contiguous [B, d]
// row images (u_img: the slots' own rows; v_img: the candidates'), the slots' two mask ids as int32 and a per-candidate
// logit offset lq, all padded to whole tiles of 32 slots; see inbatch.hip for the passes and the k order.
#pragma once
#include "refsum.hpp"
#include <cmath>

namespace inbatch {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kTile = 32;        // slots per tile: the rows and the columns of the matrix instruction
constexpr int kMaxD = 256;
constexpr int kMinGroup = 32, kMaxGroup = 4096;

// row of the 32 x 32 accumulator that register `reg` of lane half h holds (the column is lane & 31)
__device__ __forceinline__ int acc_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

// ------------------------------------------------------------------ score tiles --------------------------------------------
// The owned tile in LDS: 32 rows of 2 nq float4 chunks (zero beyond the row's d4 chunks and beyond the batch), rows
// 2 nq + 1 float4 apart so that the 16-byte reads of a half wavefront spread over the banks.
__device__ __forceinline__ void load_owned_tile(float4* __restrict__ tile, const float4* __restrict__ img, int64_t row0,
                                                int64_t batch, int d4, int nq) {
    const int per_row = 2 * nq, stride = per_row + 1;
    for (int i = mi_lane(); i < kTile * per_row; i += MI_WAVE) {
        const int r = i / per_row, ch = i - r * per_row;
        const bool in = row0 + r < batch && ch < d4;
        tile[r * stride + ch] = in ? img[(row0 + r) * d4 + ch] : mi_f4_zero();
    }
}

// acc[reg] = <streamed row row0 + acc_row(reg, h), owned row of lane & 31>.  The streamed rows are the A operand, read from
// the image (a row past the batch reads as zero), the owned rows the B operand from LDS.
__device__ __forceinline__ f32x16 score_tile(const float4* __restrict__ img, int64_t row0, int64_t batch, int d4, int nq,
                                             const float4* __restrict__ tile) {
    const int lane = mi_lane(), c = lane & 31, h = lane >> 5;
    const bool live = row0 + c < batch;
    const float4* ap = img + (live ? row0 + c : batch - 1) * d4;
    const float4* bp = tile + c * (2 * nq + 1);
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    for (int q = 0; q < nq; ++q) {
        const int ch = 2 * q + h;
        const float4 a = (live && ch < d4) ? ap[ch] : mi_f4_zero();
        const float4 b = bp[ch];
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
    }
    return acc;
}

// ------------------------------------------------------------------ 2. row statistics --------------------------------------
// One wavefront per 32 user slots.  Lane (c, h) keeps the running maximum and sum of user b0 + c over the candidates its
// half sees (rows 4h..4h+3 of every 8 of each candidate tile, tiles ascending); the halves are merged at the end, half 0 first.
static __global__ __launch_bounds__(MI_WAVE) void inbatch_stats_kernel(
    int64_t batch, int group, int d4, int nq, const float4* __restrict__ u_img, const float4* __restrict__ v_img,
    const int32_t* __restrict__ uid, const int32_t* __restrict__ pid, const float* __restrict__ lq,
    float* __restrict__ lse_out, float* __restrict__ term_out) {
    extern __shared__ float4 tile[];
    const int lane = mi_lane(), c = lane & 31, h = lane >> 5;
    const int64_t b0 = (int64_t)blockIdx.x * kTile;
    const int64_t g0 = b0 / group * group, g1 = min(g0 + group, batch);
    load_owned_tile(tile, u_img, b0, batch, d4, nq);
    __syncthreads();
    const int64_t b = b0 + c;
    const int64_t bb = min(b, batch - 1);
    const int32_t my_u = uid[bb], my_p = pid[bb];
    const float ninf = -INFINITY;
    float m = ninf, s = 0.f, diag = ninf;
    for (int64_t j0 = g0; j0 < g1; j0 += kTile) {
        const f32x16 acc = score_tile(v_img, j0, batch, d4, nq, tile);
        float x[16];
        float tmax = ninf;
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
                tmax = fmaxf(tmax, x[4 * q4 + i]);
                if (j == b) diag = l;
            }
        }
        if (tmax > ninf) {
            const float mn = fmaxf(m, tmax);
            s *= expf(m - mn);             // m = -inf: s is 0 and stays 0
#pragma unroll
            for (int i = 0; i < 16; ++i) s += expf(x[i] - mn);   // a masked candidate adds exp(-inf) = 0
            m = mn;
        }
    }
    const float mo = __shfl_xor(m, 32, MI_WAVE), so = __shfl_xor(s, 32, MI_WAVE);
    const float m_lo = h ? mo : m, m_hi = h ? m : mo, s_lo = h ? so : s, s_hi = h ? s : so;
    diag = fmaxf(diag, __shfl_xor(diag, 32, MI_WAVE));
    if (b < batch && h == 0) {   // the slot itself is never masked: the maximum is finite
        const float mx = fmaxf(m_lo, m_hi);
        const float sum = s_lo * expf(m_lo - mx) + s_hi * expf(m_hi - mx);
        const float lse = mx + logf(sum);
        lse_out[b] = lse;
        term_out[b] = lse - diag;
    }
}

// ------------------------------------------------------------------ 3. gradient sweeps -------------------------------------
// blockIdx.y = 0: the owned slots are users (dL/df[users_b] = sum_j c[b,j] f[pos_j], streamed rows = positives);
// blockIdx.y = 1: the owned slots are positives (dL/df[pos_j] = sum_b c[b,j] f[users_b], streamed rows = users).
// The coefficient tile cf has the streamed slot in its registers and the owned slot on its lane; step s of the gradient product
// takes register s as the A operand (k = lane half h <-> streamed row acc_row(s, h)) and, as the B operand, 32 columns of
// that streamed row: out[n][reg] += cf * row.  NT = the 32-column tiles of a row.
template <int NT>
static __global__ __launch_bounds__(MI_WAVE) void inbatch_sweep_kernel(
    int64_t batch, int group, int d, int nq, const float4* __restrict__ u_img, const float4* __restrict__ v_img,
    const int32_t* __restrict__ uid, const int32_t* __restrict__ pid, const float* __restrict__ lq,
    const float* __restrict__ lse, float w /* g_scale / B */, float* __restrict__ g_slot /* [2B, d]: users, positives */) {
    extern __shared__ float4 tile[];
    const int lane = mi_lane(), c = lane & 31, h = lane >> 5;
    const int d4 = d / 4;
    const bool own_user = blockIdx.y == 0;
    const float4* own = own_user ? u_img : v_img;
    const float4* str = own_user ? v_img : u_img;
    const int64_t o0 = (int64_t)blockIdx.x * kTile;
    const int64_t g0 = o0 / group * group, g1 = min(g0 + group, batch);
    load_owned_tile(tile, own, o0, batch, d4, nq);
    __syncthreads();
    const int64_t o = o0 + c;
    const int64_t oo = min(o, batch - 1);
    const int32_t my_u = uid[oo], my_p = pid[oo];
    const float my_lq = lq[oo], my_lse = lse[oo];
    f32x16 out[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int i = 0; i < 16; ++i) out[n][i] = 0.f;
    const float* strf = reinterpret_cast<const float*>(str);
    for (int64_t r0 = g0; r0 < g1; r0 += kTile) {
        const f32x16 acc = score_tile(str, r0, batch, d4, nq, tile);
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
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const int64_t r = r0 + acc_row(s, h);
            const bool live = r < batch;
            const float* row = strf + (live ? r : batch - 1) * d;
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                const int k = n * 32 + c;
                const float x = (live && k < d) ? row[k] : 0.f;
                out[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(cf[s], x, out[n], 0, 0, 0);
            }
        }
    }
    float* dst = g_slot + (own_user ? 0 : batch * d);
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        const int k = n * 32 + c;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int64_t orow = o0 + acc_row(i, h);
            if (orow < batch && k < d) dst[orow * d + k] = out[n][i];
        }
    }
}
// The chunk pass of refsum.hpp with one term per reference, the slot row itself, unweighted.
struct SlotRow {
    static constexpr int kTerms = 1;
    int64_t src = 0;   // row of g_slot
    __device__ __forceinline__ int64_t row(int, int q) const { return __shfl(src, q, MI_WAVE); }
    __device__ __forceinline__ float weight(int, int) const { return 1.f; }
};

}  // namespace inbatch
