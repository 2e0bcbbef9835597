// What the kernels that sweep users x items score tiles share (topk.hip: select the k best; rank.hip: count the items that
// beat one target): the order on scores and the loaders of a 64-row panel of a K-contiguous operand.
#pragma once
#include "common.hpp"

namespace {

__device__ __forceinline__ uint32_t score_key(float x) {
    x = x + 0.0f;  // -0 -> +0 so that equal scores compare equal
    uint32_t u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);  // monotone: larger float -> larger key
}
__device__ __forceinline__ float key_score(uint32_t k) {
    uint32_t u = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
    return __uint_as_float(u);
}

__device__ __forceinline__ unsigned long long composite(uint32_t key, uint32_t item) {
    return ((unsigned long long)key << 32) | (unsigned long long)(0xFFFFFFFFu - item);  // key desc, then id asc
}

typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int FM = 64, FN = 64, FKC = 128, FKPAD = 129;   // query / item panel rows, panel width, padded LDS row

// 64 x FKC panel rows [row0, row0 + 64) of a K-contiguous operand into registers / LDS (zero beyond n_rows and d).
__device__ __forceinline__ void fpanel_issue(float4 (&v)[8], const float* __restrict__ base, int64_t ld,
                                             const int64_t* __restrict__ row_map, int64_t row0, int64_t n_rows, int d,
                                             int tid) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int idx = tid + 256 * j;
        const int r = idx / (FKC / 4), c4 = idx % (FKC / 4);
        const int64_t gr = row0 + r;
        v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (gr < n_rows && c4 * 4 < d) {
            const int64_t row = row_map ? row_map[gr] : gr;
            v[j] = *reinterpret_cast<const float4*>(base + row * ld + c4 * 4);
        }
    }
}
// (A/B, round 1: one float per lane and load -> conflict-free LDS writes but 32 address computations spill;
// rotating the float4 component by lane / 8 -> 32 distinct banks but the selects cost more than the conflicts:
// 2.01 -> 1.71 M users/s; 132-float rows with ds_write_b128 / ds_read_b128 (conflict-free both ways, one float4
// per two MFMAs) plus a float compare against the threshold: 950 -> 1 010 us per chunk.  Stage timings of top-K's
// generic kernel per 2 621-query chunk: MFMA loop + barriers alone 586 us (114 TF/s), + panel prefetch / commit 721,
// + threshold epilogue and staging 950.  A 128-item panel with two accumulators per wavefront (one workgroup per CU):
// 2.06 -> 1.74 M users/s.  The plain four-word write below stays.)
__device__ __forceinline__ void fpanel_commit(float (*panel)[FKPAD], const float4 (&v)[8], int tid) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int idx = tid + 256 * j;
        const int r = idx / (FKC / 4), c = (idx % (FKC / 4)) * 4;
        panel[r][c] = v[j].x; panel[r][c + 1] = v[j].y; panel[r][c + 2] = v[j].z; panel[r][c + 3] = v[j].w;
    }
}

}  // namespace

// CUs of the current device (the grid rules of the fused kernels: workgroups per round of the chip)
static int mi_cu_count() {
    static int n_cu = 0;
    if (n_cu == 0) {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) n_cu = v;
        else n_cu = 256;
    }
    return n_cu;
}
