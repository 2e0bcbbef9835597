// The 32 x 32 score tiles of the losses that score on the exact-f32 matrix instruction (v_mfma_f32_32x32x2_f32: bit for bit a
// k-ordered fmaf chain): the in-batch softmax and the contrastive term (inbatch_tiles.hpp) and the full-catalogue softmax
// (fullsoftmax.hip).  A wavefront OWNS 32 rows, which sit on its lanes (the B operand, staged once in LDS), while the other
// side's rows STREAM past as the A operand; the scores never leave the registers, and every pass that needs them computes
// them again.  What the passes of every one of these losses must agree on is written here and nowhere else:
//   lane map       lane = (c, h), c = lane & 31 the owned row, h = lane >> 5 the half; register reg of a tile holds the
//                  streamed row acc_row(reg, h): registers 4 g .. 4 g + 3 are the consecutive rows 8 g + 4 h .. 8 g + 4 h + 3
//   k order        half h takes the float4 chunks 2 q + h of a row, q ascending, the four floats in order, and the instruction
//                  adds half 0's product before half 1's.  A product of two floats does not depend on which side owns, so
//                  every pass sees the same score bits for a pair of rows
//   rescale order  a lane's running (max, sum) takes a tile's sixteen logits at once, registers ascending, and the two
//                  halves are merged half 0 first (lse_add_tile, lse_fold_halves)
#pragma once
#include "common.hpp"
#include <cmath>

namespace loss_tiles {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kTile = 32;        // rows per tile: the rows and the columns of the matrix instruction
constexpr int kMaxD = 256;

// row of the 32 x 32 accumulator that register `reg` of lane half h holds (the column is lane & 31)
__device__ __forceinline__ int acc_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

// A side of the score block: n rows of d4 float4 chunks, ld4 float4 apart (a contiguous [B, d] image, or rows of a table).
struct Rows {
    const float4* __restrict__ p;
    int64_t ld4, n;
};

// ------------------------------------------------------------------ score tiles --------------------------------------------
// The owned tile in LDS: 32 rows of 2 nq float4 chunks (zero beyond the row's d4 chunks and beyond the side's rows), rows
// 2 nq + 1 float4 apart so that the 16-byte reads of a half wavefront spread over the banks.
__device__ __forceinline__ void load_owned_tile(float4* __restrict__ tile, const Rows& own, int64_t row0, int d4, int nq) {
    const int per_row = 2 * nq, stride = per_row + 1;
    for (int i = mi_lane(); i < kTile * per_row; i += MI_WAVE) {
        const int r = i / per_row, ch = i - r * per_row;
        const bool in = row0 + r < own.n && ch < d4;
        tile[r * stride + ch] = in ? own.p[(row0 + r) * own.ld4 + ch] : mi_f4_zero();
    }
}

// float4 chunk ch of a streamed row: zero past the row's d4 chunks and where the row is past the side's end
__device__ __forceinline__ float4 a_chunk(const float4* __restrict__ row, bool live, int ch, int d4) {
    return (live && ch < d4) ? row[ch] : mi_f4_zero();
}

// acc[reg] = <streamed row row0 + acc_row(reg, h), owned row of lane & 31>.  The streamed rows are read from memory (a row
// past the side's end reads as zero), the owned rows from LDS.  nq k steps, a multiple of kLoadGroup (the chunks past d4 are
// zero on both sides and add exact zeros).  kLoadGroup = 1 loads a step's A chunk where it is used.  A larger group loads its
// steps' A chunks together (at 4, one 128-byte line of a row over the two halves) and one group ahead, the next group's while
// this group's matrix instructions run: the choice of a pass that streams far more tiles than fit the caches.
template <int kLoadGroup>
__device__ __forceinline__ f32x16 score_tile(const Rows& str, int64_t row0, int d4, int nq, const float4* __restrict__ tile) {
    constexpr bool kAhead = kLoadGroup > 1;
    const int lane = mi_lane(), c = lane & 31, h = lane >> 5;
    const bool live = row0 + c < str.n;
    const float4* ap = str.p + (live ? row0 + c : str.n - 1) * str.ld4;
    const float4* bp = tile + c * (2 * nq + 1);
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    float4 cur[kLoadGroup], nxt[kLoadGroup];
    if (kAhead) {
#pragma unroll
        for (int u = 0; u < kLoadGroup; ++u) {
            cur[u] = a_chunk(ap, live, 2 * u + h, d4);
            nxt[u] = mi_f4_zero();
        }
    }
    for (int q0 = 0; q0 < nq; q0 += kLoadGroup) {
        if (!kAhead) {
            cur[0] = a_chunk(ap, live, 2 * q0 + h, d4);
        } else if (q0 + kLoadGroup < nq) {
#pragma unroll
            for (int u = 0; u < kLoadGroup; ++u) nxt[u] = a_chunk(ap, live, 2 * (q0 + kLoadGroup + u) + h, d4);
        }
#pragma unroll
        for (int u = 0; u < kLoadGroup; ++u) {
            const float4 a = cur[u];
            const float4 b = bp[2 * (q0 + u) + h];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
        }
        if (kAhead) {
#pragma unroll
            for (int u = 0; u < kLoadGroup; ++u) cur[u] = nxt[u];
        }
    }
    return acc;
}

// ------------------------------------------------------------------ row statistics -----------------------------------------
// The running maximum m and sum s (of exp(x - m)) of owned row c over the streamed rows that lane (c, h) has seen: rows
// 4h .. 4h + 3 of every 8 of each tile.  x holds a tile's sixteen logits, a masked one as -inf, which adds exp(-inf) = 0.
struct MaxSum {
    float m = -INFINITY, s = 0.f;
};

__device__ __forceinline__ void lse_add_tile(MaxSum& run, const float (&x)[16]) {
    float tmax = -INFINITY;
#pragma unroll
    for (int i = 0; i < 16; ++i) tmax = fmaxf(tmax, x[i]);
    if (tmax > -INFINITY) {
        const float mn = fmaxf(run.m, tmax);
        run.s *= expf(run.m - mn);             // m = -inf: s is 0 and stays 0
#pragma unroll
        for (int i = 0; i < 16; ++i) run.s += expf(x[i] - mn);
        run.m = mn;
    }
}

// The two halves' pairs of an owned row merged, half 0 first: (max, sum of exp(x - max)) over every streamed row seen.  Half 0
// gets the pair; at least one of the two maxima must be finite.
__device__ __forceinline__ MaxSum lse_fold_halves(const MaxSum& run, int h) {
    const float mo = __shfl_xor(run.m, 32, MI_WAVE), so = __shfl_xor(run.s, 32, MI_WAVE);
    const float m_lo = h ? mo : run.m, m_hi = h ? run.m : mo, s_lo = h ? so : run.s, s_hi = h ? run.s : so;
    MaxSum all;
    all.m = fmaxf(m_lo, m_hi);
    all.s = s_lo * expf(m_lo - all.m) + s_hi * expf(m_hi - all.m);
    return all;
}

// ------------------------------------------------------------------ gradient product ---------------------------------------
// out[n][reg] = d(loss) / d(owned row acc_row(reg, h))[32 n + c], summed over the streamed tiles.  A coefficient tile cf has
// the streamed row in its registers and the owned row on its lane, like a score tile: it is the A operand of the product as
// it stands (the sum runs over the accumulator's row index), no transpose, no LDS.  Step s takes register s (k = lane half h
// <-> streamed row acc_row(s, h)) and, as the B operand, 32 columns of that streamed row.  NT = the 32-column tiles of a row.
template <int NT>
__device__ __forceinline__ void grad_zero(f32x16 (&out)[NT]) {
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int i = 0; i < 16; ++i) out[n][i] = 0.f;
}

template <int NT>
__device__ __forceinline__ void grad_add_tile(f32x16 (&out)[NT], const f32x16& cf, const Rows& str, int64_t r0, int d) {
    const int lane = mi_lane(), c = lane & 31, h = lane >> 5;
    const float* strf = reinterpret_cast<const float*>(str.p);
    const int64_t str_ld = str.ld4 * 4;
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        const int64_t r = r0 + acc_row(s, h);
        const bool live = r < str.n;
        const float* row = strf + (live ? r : str.n - 1) * str_ld;
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            const int k = n * 32 + c;
            const float x = (live && k < d) ? row[k] : 0.f;
            out[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(cf[s], x, out[n], 0, 0, 0);
        }
    }
}

// The owned rows o0 .. o0 + 31 below n_own, d floats each, to rows of dst that lie ldd floats apart: one writer per row.
template <int NT>
__device__ __forceinline__ void grad_store(const f32x16 (&out)[NT], float* __restrict__ dst, int64_t ldd, int64_t o0,
                                           int64_t n_own, int d) {
    const int lane = mi_lane(), c = lane & 31, h = lane >> 5;
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        const int k = n * 32 + c;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int64_t orow = o0 + acc_row(i, h);
            if (orow < n_own && k < d) dst[orow * ldd + k] = out[n][i];
        }
    }
}

// ------------------------------------------------------------------ gather -------------------------------------------------
// One float4 step of a slot's L2 term: rg + the squares of x's four floats, then of y's, one fmaf each, in order.
__device__ __forceinline__ float add_squares(float rg, const float4& x, const float4& y) {
    rg = fmaf(x.x, x.x, rg); rg = fmaf(x.y, x.y, rg); rg = fmaf(x.z, x.z, rg); rg = fmaf(x.w, x.w, rg);
    rg = fmaf(y.x, y.x, rg); rg = fmaf(y.y, y.y, rg); rg = fmaf(y.z, y.z, rg); rg = fmaf(y.w, y.w, rg);
    return rg;
}

}  // namespace loss_tiles
