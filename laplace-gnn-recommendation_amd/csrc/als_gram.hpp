// The rank-n update of the implicit-ALS row solves, shared by csrc/als.hip (one system per row) and csrc/als_block.hip (the
// hub rows of the block solver): width classes, the deal of the lower-triangle tiles to the wavefronts, and the gather /
// MFMA loop that forms (S_c, s_c) of one chunk of a row.  The layout is described at the top of csrc/als.hip; the order of
// every sum is the "iALS" / "iALS weighted" rule of include/laplace_hip.h.  `A` is the caller's argument struct: d, n_cols,
// idx, Y, ldy (and conf for the weighted form) are read from it.
#pragma once
#include "common.hpp"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int ALS_KT = 32;   // entries staged per step

template <int DP_, int WAVES_>
struct AlsCfg {
    static constexpr int DP = DP_, WAVES = WAVES_;
    static constexpr int NT = WAVES * 64;
    static constexpr int TD = DP / 16;
    static constexpr int NTILES = TD * (TD + 1) / 2;
    static constexpr int TPW = (NTILES + WAVES - 1) / WAVES;
    static constexpr int LDA = DP == 16 ? 16 : DP + 16;
    static constexpr int F4 = DP / 4;
    static constexpr int U = ALS_KT * F4 / NT;
    static constexpr int SM_ROWS = (DP + 1) > ALS_KT ? (DP + 1) : ALS_KT;
    static constexpr int SM_ROWS_W = (DP + 1) > 2 * ALS_KT ? (DP + 1) : 2 * ALS_KT;   // weighted: a second staged image (z)
    static_assert(ALS_KT * F4 % NT == 0, "whole float4 slots per thread");
};

__device__ __forceinline__ void als_tile_of(int q, int& ti, int& tj) {
    ti = 0;
    while ((ti + 1) * (ti + 2) / 2 <= q) ++ti;
    tj = q - ti * (ti + 1) / 2;
}

// (S_c, s_c) of entries [p0, p1) of idx: acc[s] is tile (ti[s], tj[s]) in the MFMA's C layout (column lane & 15, rows 4 (lane >> 4)
// + reg), s_sum is column tid of s (tid < d).  Ends behind a barrier: the caller may overwrite `stage`.
template <class C, class A>
__device__ __forceinline__ void als_accumulate(const A& a, int p0, int p1, float* stage, const int (&ti)[C::TPW],
                                               const int (&tj)[C::TPW], const bool (&live)[C::TPW], f32x4 (&acc)[C::TPW],
                                               float& s_sum) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int d = a.d;
    float4 pre[C::U];
    auto fetch = [&](int q0) {
#pragma unroll
        for (int u = 0; u < C::U; ++u) {
            const int f = tid + C::NT * u, e = f / C::F4, c4 = f % C::F4;
            float4 v = mi_f4_zero();
            if (q0 + e < p1 && 4 * c4 < d) {
                const int col = a.idx[q0 + e];
                if ((unsigned)col < (unsigned)a.n_cols) v = *reinterpret_cast<const float4*>(a.Y + (int64_t)col * a.ldy + 4 * c4);
            }
            pre[u] = v;
        }
    };
    fetch(p0);
    const int arow = lane >> 4, acol = lane & 15;
    for (int q0 = p0; q0 < p1; q0 += ALS_KT) {
#pragma unroll
        for (int u = 0; u < C::U; ++u) {
            const int f = tid + C::NT * u, e = f / C::F4, c4 = f % C::F4;
            *reinterpret_cast<float4*>(stage + e * C::LDA + 4 * c4) = pre[u];
        }
        __syncthreads();
        if (q0 + ALS_KT < p1) fetch(q0 + ALS_KT);
        const int ne = min(ALS_KT, p1 - q0), steps = (ne + 3) >> 2;
        for (int ks = 0; ks < steps; ++ks) {
            const float* row = stage + (4 * ks + arow) * C::LDA + acol;
#pragma unroll
            for (int s = 0; s < C::TPW; ++s) {
                if (live[s]) acc[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(row[16 * ti[s]], row[16 * tj[s]], acc[s], 0, 0, 0);
            }
        }
        if (tid < d) {
            for (int e = 0; e < ne; ++e) s_sum += stage[e * C::LDA + tid];
        }
        __syncthreads();
    }
}

// The weighted sibling ("iALS weighted" in the header): S_c[j][k] = sum_e y_e[j] z_e[k] with z_e = a_e * y_e (one f32 product per
// element, made once while staging), s_c[j] = sum_e c_e y_e[j] with c_e = 1.0f + a_e.  `stage` holds TWO images of ALS_KT
// rows, y then z, both with the stride C::LDA: the A operand of tile (ti, tj) is read from y, the B operand from z.  a_e comes
// in with the same ALS_KT prefetch as idx; an entry past the end of the row is staged as y = z = 0 with c = 0.
template <class C, class A>
__device__ __forceinline__ void als_accumulate_w(const A& a, int p0, int p1, float* stage, float* cs, const int (&ti)[C::TPW],
                                                 const int (&tj)[C::TPW], const bool (&live)[C::TPW], f32x4 (&acc)[C::TPW],
                                                 float& s_sum) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int d = a.d;
    float* stagez = stage + ALS_KT * C::LDA;
    float4 pre[C::U];
    float prea[C::U];
    auto fetch = [&](int q0) {
#pragma unroll
        for (int u = 0; u < C::U; ++u) {
            const int f = tid + C::NT * u, e = f / C::F4, c4 = f % C::F4;
            float4 v = mi_f4_zero();
            float w = 0.f;
            if (q0 + e < p1) {
                w = a.conf[q0 + e];
                if (4 * c4 < d) {
                    const int col = a.idx[q0 + e];
                    if ((unsigned)col < (unsigned)a.n_cols) v = *reinterpret_cast<const float4*>(a.Y + (int64_t)col * a.ldy + 4 * c4);
                }
            }
            pre[u] = v;
            prea[u] = w;
        }
    };
    fetch(p0);
    const int arow = lane >> 4, acol = lane & 15;
    for (int q0 = p0; q0 < p1; q0 += ALS_KT) {
#pragma unroll
        for (int u = 0; u < C::U; ++u) {
            const int f = tid + C::NT * u, e = f / C::F4, c4 = f % C::F4;
            const float4 v = pre[u];
            const float w = prea[u];
            *reinterpret_cast<float4*>(stage + e * C::LDA + 4 * c4) = v;
            *reinterpret_cast<float4*>(stagez + e * C::LDA + 4 * c4) = make_float4(w * v.x, w * v.y, w * v.z, w * v.w);
            if (c4 == 0) cs[e] = q0 + e < p1 ? 1.0f + w : 0.f;
        }
        __syncthreads();
        if (q0 + ALS_KT < p1) fetch(q0 + ALS_KT);
        const int ne = min(ALS_KT, p1 - q0), steps = (ne + 3) >> 2;
        for (int ks = 0; ks < steps; ++ks) {
            const float* row = stage + (4 * ks + arow) * C::LDA + acol;
            const float* rowz = stagez + (4 * ks + arow) * C::LDA + acol;
#pragma unroll
            for (int s = 0; s < C::TPW; ++s) {
                if (live[s]) acc[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(row[16 * ti[s]], rowz[16 * tj[s]], acc[s], 0, 0, 0);
            }
        }
        if (tid < d) {
            for (int e = 0; e < ne; ++e) s_sum = fmaf(cs[e], stage[e * C::LDA + tid], s_sum);
        }
        __syncthreads();
    }
}

template <class C>
__device__ __forceinline__ void als_tiles(int d, int (&ti)[C::TPW], int (&tj)[C::TPW], bool (&live)[C::TPW]) {
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int s = 0; s < C::TPW; ++s) {
        const int q = wave + C::WAVES * s;
        ti[s] = tj[s] = 0;
        live[s] = q < C::NTILES;
        if (live[s]) {
            als_tile_of(q, ti[s], tj[s]);
            live[s] = 16 * ti[s] < d;   // tj <= ti
        }
    }
}

}  // namespace
