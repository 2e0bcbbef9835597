// N5: PinSAGE's item feature projector (mi_pinsage_project_f32 / _bwd_f32 / _clear_f32; include/laplace_hip.h, ABI 14).
//
//   out[r] = id_table[i] + tables[0][x[i, 0]] + ... + tables[C - 1][x[i, C - 1]] + (dense[i] @ w^T + b),   i = ids ? ids[r] : r
//
// one f32 addition chain in that order (restates the reference's LinearProjector, pinsage/layers.py:14-46, 90-118: a
// projection per feature column, summed).  The table part is a gather kernel, one lane per float4 of an output row; the
// dense part goes through the f32-MFMA launcher (gemm.hpp) with its row gather, accumulating into `out`.
//
// Backward.  A categorical column has tens of values, so at the executor's largest block one code is looked up by
// thousands of rows, from every workgroup of any row-parallel grid: the table gradient is a segmented sum with very long
// segments.  proj_refs_kernel writes one reference per (slot, r) — key (slot, code), the columns then the id, payload r — in
// slot-major order, then ascending r, and segsum.hpp sums the rows of g by key in that order (stable sort, chunks of 64,
// segsum::chunk_kernel / segsum::combine_kernel): one writer per row, a fixed association, no float atomics.  g_b is a
// fixed-order column sum (128-row slabs, then the slabs in order); g_w = g^T @ dense[ids] is a trans_a product on the
// launcher (split-K under its rule) over the gathered rows.
#include "gemm.hpp"
#include "segsum.hpp"
#include "lazy_adam.hpp"

namespace {

constexpr int kBlock = 256;
constexpr int kSlab = 128;       // rows per partial of the g_b column sum
constexpr int kMaxSlots = MI_PROJECTOR_MAX_COLS + 1;   // the columns, then the id

inline unsigned grid_for(int64_t n) { return (unsigned)mi_ceil_div(n > 0 ? n : 1, kBlock); }

using ProjTables = segsum::Ptrs<const float4, kMaxSlots>;   // by value in the kernel arguments
using ProjGradTables = segsum::Ptrs<float4, kMaxSlots>;

// ---- forward ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void proj_gather_kernel(int64_t n, int h4, int n_cols, const int64_t* __restrict__ ids,
                                                             const int64_t* __restrict__ x, const float4* __restrict__ id_table,
                                                             ProjTables tabs, float4* __restrict__ out, int64_t ldo4) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n * h4) return;
    const int64_t r = i / h4;
    const int e = (int)(i - r * h4);
    const int64_t item = ids ? ids[r] : r;
    int64_t code[MI_PROJECTOR_MAX_COLS];
#pragma unroll
    for (int c = 0; c < MI_PROJECTOR_MAX_COLS; ++c) code[c] = c < n_cols ? x[item * n_cols + c] : 0;
    float4 row[MI_PROJECTOR_MAX_COLS];
#pragma unroll
    for (int c = 0; c < MI_PROJECTOR_MAX_COLS; ++c)
        row[c] = c < n_cols ? tabs.t[c][code[c] * h4 + e] : mi_f4_zero();
    float4 acc = mi_f4_zero();
    bool first = true;
    if (id_table) {
        acc = id_table[item * h4 + e];
        first = false;
    }
#pragma unroll
    for (int c = 0; c < MI_PROJECTOR_MAX_COLS; ++c) {   // no early exit: the arrays stay in registers
        if (c < n_cols) {
            acc = first ? row[c] : mi_f4_add(acc, row[c]);
            first = false;
        }
    }
    out[r * ldo4 + e] = acc;
}

// ---- backward: references ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void proj_refs_kernel(int64_t n, int64_t n_ref, int n_cols, const int64_t* __restrict__ ids,
                                                           const int64_t* __restrict__ x, unsigned shift,
                                                           uint64_t* __restrict__ keys, uint32_t* __restrict__ refs) {
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;   // reference = slot * n + r
    if (j >= n_ref) return;
    const int64_t slot = j / n, r = j - slot * n;
    const int64_t item = ids ? ids[r] : r;
    const int64_t code = slot < n_cols ? x[item * n_cols + slot] : item;
    keys[j] = ((uint64_t)slot << shift) | (uint64_t)code;
    refs[j] = (uint32_t)r;   // the payload is the row of g to add; the initial order (slot, then r) is what the stable sort keeps
}

// The rows the backward wrote, back to zero (every writer stores the same zeros).
__global__ __launch_bounds__(kBlock) void proj_clear_kernel(int64_t n, int64_t n_ref, int h4, int n_cols,
                                                            const int64_t* __restrict__ ids, const int64_t* __restrict__ x,
                                                            ProjGradTables gt) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_ref * h4) return;
    const int64_t j = i / h4;
    const int e = (int)(i - j * h4);
    const int64_t slot = j / n, r = j - slot * n;
    const int64_t item = ids ? ids[r] : r;
    const int64_t code = slot < n_cols ? x[item * n_cols + slot] : item;
    gt.at((int)slot)[code * h4 + e] = mi_f4_zero();
}

// ---- backward: g_b, a fixed-order column sum -------------------------------------------------------------------------------
__global__ __launch_bounds__(128) void proj_colsum_slab_kernel(int64_t n, int h, const float* __restrict__ g, int64_t ldg,
                                                               float* __restrict__ part) {
    const int c = threadIdx.x;
    if (c >= h) return;
    const int64_t r0 = (int64_t)blockIdx.x * kSlab, r1 = min(n, r0 + kSlab);
    float s = 0.f;
#pragma unroll 8
    for (int64_t r = r0; r < r1; ++r) s += g[r * ldg + c];
    part[(int64_t)blockIdx.x * h + c] = s;
}
__global__ __launch_bounds__(128) void proj_colsum_final_kernel(int64_t n_slabs, int h, const float* __restrict__ part,
                                                                float* __restrict__ out) {
    const int c = threadIdx.x;
    if (c >= h) return;
    float s = 0.f;
#pragma unroll 8
    for (int64_t b = 0; b < n_slabs; ++b) s += part[b * h + c];
    out[c] = s;
}

// dst[r, 0 .. ldd) = dense[ids[r], 0 .. f), zero beyond f
__global__ __launch_bounds__(kBlock) void proj_gather_dense_kernel(int64_t n, int64_t f, int64_t ldd, const int64_t* __restrict__ ids,
                                                                   const float* __restrict__ dense, int64_t ld,
                                                                   float* __restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n * ldd) return;
    const int64_t r = i / ldd, k = i - r * ldd;
    dst[i] = k < f ? dense[ids[r] * ld + k] : 0.f;
}

// ---- host ------------------------------------------------------------------------------------------------------------------
inline int n_slots(const mi_item_projector& p) { return p.n_cols + (p.id_table ? 1 : 0); }

// Everything about the descriptor that does not depend on the call's buffers.  0, or the code to return.
int check_projector(const mi_item_projector* pp, int64_t n, bool has_ids) {
    if (!pp) return MI_ERR_BAD_ARG;
    const mi_item_projector& p = *pp;
    if (p.hidden < 4 || p.hidden % 4 != 0 || p.hidden > 128) return MI_ERR_UNSUPPORTED;
    if (p.n_cols > MI_PROJECTOR_MAX_COLS) return MI_ERR_UNSUPPORTED;
    if (p.n_cols < 0 || p.n_dense < 0 || p.n_items < 1 || n < 0) return MI_ERR_BAD_ARG;
    if (!has_ids && n > p.n_items) return MI_ERR_BAD_ARG;
    if (p.n_cols == 0 && p.n_dense == 0 && !p.id_table) return MI_ERR_BAD_ARG;
    if (p.n_cols > 0 && !p.x) return MI_ERR_BAD_ARG;
    for (int c = 0; c < p.n_cols; ++c) {
        if (!p.tables[c] || !mi_aligned16(p.tables[c]) || p.table_rows[c] < 1) return MI_ERR_BAD_ARG;
        if (p.table_rows[c] >= ((int64_t)1 << 40)) return MI_ERR_TOO_LARGE;
    }
    if (p.id_table && !mi_aligned16(p.id_table)) return MI_ERR_BAD_ARG;
    if (p.n_items >= ((int64_t)1 << 40)) return MI_ERR_TOO_LARGE;
    if (p.n_dense > 0 && (!p.dense || !p.w || !p.b || p.ld_dense < p.n_dense)) return MI_ERR_BAD_ARG;
    if (n * (int64_t)std::max(1, n_slots(p)) >= INT32_MAX || p.n_dense >= INT32_MAX) return MI_ERR_TOO_LARGE;
    return 0;
}

// The launcher's split-K workspace for an [m, n_out] product over k, as a bound that never shrinks when m grows (fewer
// slices are cut as the tile grid fills: the raw need is not monotone).
size_t gemm_ws_upto(int64_t m, int64_t n_out, int64_t k) {
    size_t best = 0;
    for (int64_t tiles = 1; tiles <= 128; ++tiles) {
        const int64_t mm = std::min(m, tiles * 64);
        if (mm <= 0) break;
        best = std::max(best, mi_gemm_workspace_bytes(mm, n_out, k));
        if (mm == m) break;
    }
    return best;
}

size_t sort_tmp_cap(int64_t n_ref) { return ((size_t)2 << 20) + mi_align_up((size_t)n_ref * 4, 256); }

size_t fwd_ws_bytes(const mi_item_projector& p, int64_t n) {
    return 256 + (p.n_dense > 0 ? gemm_ws_upto(n, p.hidden, p.n_dense) : 0);
}

struct BwdSizes {
    int64_t n_ref, n_slabs, ldd;
};
BwdSizes bwd_sizes(const mi_item_projector& p, int64_t n) {
    BwdSizes z;
    z.n_ref = n * n_slots(p);
    z.n_slabs = mi_ceil_div(n, kSlab);
    z.ldd = (p.n_dense + 3) / 4 * 4;
    return z;
}
size_t bwd_ws_bytes(const mi_item_projector& p, int64_t n) {
    const BwdSizes z = bwd_sizes(p, n);
    size_t total = 256 + segsum::workspace_bytes(z.n_ref, p.hidden, sort_tmp_cap(z.n_ref));
    if (p.n_dense > 0) {
        total += mi_align_up((size_t)std::max<int64_t>(z.n_slabs, 1) * p.hidden * sizeof(float), 256);
        total += mi_align_up((size_t)std::max<int64_t>(n, 1) * z.ldd * sizeof(float), 256);
        total += mi_align_up(mi_gemm_workspace_bytes(p.hidden, p.n_dense, n), 256);   // g_w over k = n: never fewer slices as n grows
    }
    return total;
}

ProjGradTables grad_tables(const mi_item_projector& p, const mi_item_projector_grads& gr) {
    ProjGradTables gt;
    for (int s = 0; s < kMaxSlots; ++s) gt.t[s] = nullptr;
    for (int c = 0; c < p.n_cols; ++c) gt.t[c] = reinterpret_cast<float4*>(gr.g_tables[c]);
    if (p.id_table) gt.t[p.n_cols] = reinterpret_cast<float4*>(gr.g_id_table);
    return gt;
}

int check_grads(const mi_item_projector& p, const mi_item_projector_grads* gr, bool dense_too) {
    if (!gr) return MI_ERR_BAD_ARG;
    for (int c = 0; c < p.n_cols; ++c)
        if (!gr->g_tables[c] || !mi_aligned16(gr->g_tables[c])) return MI_ERR_BAD_ARG;
    if (p.id_table && (!gr->g_id_table || !mi_aligned16(gr->g_id_table))) return MI_ERR_BAD_ARG;
    if (dense_too && p.n_dense > 0 && (!gr->g_w || !gr->g_b)) return MI_ERR_BAD_ARG;
    return 0;
}

using LazyOp = MiLazyRowOp<segsum::Ptrs<float4, kMaxSlots>>;

// The per-row operation of a lazy call.  < 0: the code to return; 0: no slot is lazy (*op not filled); 1: some slot is.
int lazy_op(const mi_item_projector& p, const mi_item_projector_moments* mo, const mi_lazy_adam* lazy, LazyOp* op) {
    if (!mo) return 0;
    bool any = false;
    for (int s = 0; s < kMaxSlots; ++s) op->p.t[s] = op->m.t[s] = op->v.t[s] = nullptr;
    auto slot = [&](int s, const float* table, float* m, float* v) -> int {
        if ((m == nullptr) != (v == nullptr)) return MI_ERR_BAD_ARG;
        if (!m) return 0;
        if (!mi_aligned16(m) || !mi_aligned16(v)) return MI_ERR_BAD_ARG;
        op->p.t[s] = reinterpret_cast<float4*>(const_cast<float*>(table));   // a lazy slot's table is written
        op->m.t[s] = reinterpret_cast<float4*>(m);
        op->v.t[s] = reinterpret_cast<float4*>(v);
        any = true;
        return 0;
    };
    for (int c = 0; c < p.n_cols; ++c) {
        const int bad = slot(c, p.tables[c], mo->m_tables[c], mo->v_tables[c]);
        if (bad) return bad;
    }
    if (p.id_table) {
        const int bad = slot(p.n_cols, p.id_table, mo->m_id_table, mo->v_id_table);
        if (bad) return bad;
    } else if (mo->m_id_table || mo->v_id_table) {
        return MI_ERR_BAD_ARG;   // moments for a table the projector does not have
    }
    if (!any) return 0;
    const int bad = mi_lazy_check(lazy);
    if (bad) return bad;
    op->c = mi_lazy_consts(*lazy);
    return 1;
}

// mi_pinsage_project_bwd_f32 (moments == nullptr) and mi_pinsage_project_bwd_lazy_f32: one body, so that the gradients are the
// same bits.  With a moment pair for some slot the lazy update runs over the heads of the sorted keys after the combine.
static int project_bwd(const mi_item_projector* pp, const mi_item_projector_grads* grads, const mi_item_projector_moments* moments,
                       const mi_lazy_adam* lazy, int64_t n, const int64_t* ids, const float* g, int64_t ldg, void* ws, size_t ws_bytes,
                       mi_stream_t stream) {
    int bad = check_projector(pp, n, ids != nullptr);
    if (bad) return bad;
    const mi_item_projector& p = *pp;
    bad = check_grads(p, grads, true);
    if (bad) return bad;
    LazyOp op = {};
    bad = lazy_op(p, moments, lazy, &op);
    if (bad < 0) return bad;
    const bool any_lazy = bad > 0;
    MI_CHECK_ARG(n == 0 || (g && mi_aligned16(g) && ldg >= p.hidden && ldg % 4 == 0));
    if (!ws || ws_bytes < bwd_ws_bytes(p, n)) return MI_ERR_WORKSPACE;
    const BwdSizes z = bwd_sizes(p, n);
    const int H = p.hidden;
    hipStream_t s = (hipStream_t)stream;
    MiArena arena(ws, ws_bytes);
    const segsum::Buffers sb = segsum::take(arena, z.n_ref, H, sort_tmp_cap(z.n_ref));
    float *slabs = nullptr, *dense_rows = nullptr;
    char* gemm_ws = nullptr;
    size_t gemm_ws_bytes = 0;
    if (p.n_dense > 0) {
        slabs = arena.take<float>((size_t)std::max<int64_t>(z.n_slabs, 1) * H);
        dense_rows = arena.take<float>((size_t)std::max<int64_t>(n, 1) * z.ldd);
        gemm_ws_bytes = mi_gemm_workspace_bytes(H, p.n_dense, n);
        gemm_ws = arena.take<char>(gemm_ws_bytes ? gemm_ws_bytes : 1);
        if (!slabs || !dense_rows || !gemm_ws) return MI_ERR_WORKSPACE;
    }
    if (!sb.ok()) return MI_ERR_WORKSPACE;
    if (z.n_ref > 0) {
        // the key: slot above `shift` bits of code (a column's code, or the item id in the last slot)
        int64_t widest = p.id_table ? p.n_items : 1;
        for (int c = 0; c < p.n_cols; ++c) widest = std::max(widest, p.table_rows[c]);
        const unsigned shift = mi_bits_for(widest), bits = shift + mi_bits_for(kMaxSlots);
        auto refs = [&]() -> int {
            hipLaunchKernelGGL(proj_refs_kernel, dim3(grid_for(z.n_ref)), dim3(kBlock), 0, s, n, z.n_ref, (int)p.n_cols, ids, p.x,
                               shift, sb.k0, sb.r0);
            return 0;
        };
        const uint64_t* sorted = nullptr;
        int rc = segsum::run<false>(sb, z.n_ref, nullptr, shift, bits, 0, refs, g, ldg, H, segsum::Plain(), grad_tables(p, *grads), s,
                                    &sorted);
        if (rc) return rc;
        if (any_lazy) {
            rc = segsum::run_heads<false>(sorted, z.n_ref, nullptr, shift, H, grad_tables(p, *grads), op, s);
            if (rc) return rc;
        }
    }
    if (p.n_dense > 0) {
        if (z.n_slabs > 0)
            hipLaunchKernelGGL(proj_colsum_slab_kernel, dim3((unsigned)z.n_slabs), dim3(128), 0, s, n, H, g, ldg, slabs);
        hipLaunchKernelGGL(proj_colsum_final_kernel, dim3(1), dim3(128), 0, s, z.n_slabs, H, slabs, grads->g_b);
        const float* rows = p.dense;
        int64_t ld_rows = p.ld_dense;
        if (ids && n > 0) {
            hipLaunchKernelGGL(proj_gather_dense_kernel, dim3(grid_for(n * z.ldd)), dim3(kBlock), 0, s, n, p.n_dense, z.ldd, ids,
                               p.dense, p.ld_dense, dense_rows);
            rows = dense_rows;
            ld_rows = z.ldd;
        }
        const int rc = mi_launch_status();
        if (rc) return rc;
        MiGemmArgs q;   // g_w[h, f] = sum_r g[r, h] * rows[r, f]
        memset(&q, 0, sizeof(q));
        q.M = H; q.N = p.n_dense; q.K = n;
        q.A = g; q.sa_m = 1; q.sa_k = ldg; q.a_rows = nullptr;
        q.B = rows; q.sb_n = 1; q.sb_k = ld_rows;
        q.bias = nullptr; q.C = grads->g_w; q.ldc = p.n_dense; q.accumulate = 0; q.act = 0;
        return mi_gemm_launch(q, gemm_ws, gemm_ws_bytes, s);
    }
    return 0;
}

}  // namespace

extern "C" {

int64_t mi_pinsage_project_sizeof(int32_t which) {
    switch (which) {
        case 0: return (int64_t)sizeof(mi_item_projector);
        case 1: return (int64_t)sizeof(mi_item_projector_grads);
        default: return -1;
    }
}

size_t mi_pinsage_project_workspace_bytes(const mi_item_projector* p, int64_t n) {
    if (check_projector(p, n, true) != 0) return 0;
    return fwd_ws_bytes(*p, n);
}

int mi_pinsage_project_f32(const mi_item_projector* pp, int64_t n, const int64_t* ids, float* out, int64_t ldo, void* ws,
                           size_t ws_bytes, mi_stream_t stream) {
    const int bad = check_projector(pp, n, ids != nullptr);
    if (bad) return bad;
    const mi_item_projector& p = *pp;
    if (n == 0) return 0;
    MI_CHECK_ARG(out && mi_aligned16(out) && ldo >= p.hidden && ldo % 4 == 0);
    const int64_t gemm_ws = p.n_dense > 0 ? (int64_t)mi_gemm_workspace_bytes(n, p.hidden, p.n_dense) : 0;
    if (gemm_ws > 0 && (!ws || ws_bytes < (size_t)gemm_ws)) return MI_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int h4 = p.hidden / 4;
    const bool tables = n_slots(p) > 0;
    if (tables) {
        ProjTables tabs;
        for (int c = 0; c < kMaxSlots; ++c) tabs.t[c] = c < p.n_cols ? reinterpret_cast<const float4*>(p.tables[c]) : nullptr;
        hipLaunchKernelGGL(proj_gather_kernel, dim3(grid_for(n * h4)), dim3(kBlock), 0, s, n, h4, (int)p.n_cols, ids, p.x,
                           reinterpret_cast<const float4*>(p.id_table), tabs, reinterpret_cast<float4*>(out), ldo / 4);
        const int rc = mi_launch_status();
        if (rc) return rc;
    }
    if (p.n_dense > 0) {
        MiGemmArgs g;
        memset(&g, 0, sizeof(g));
        g.M = n; g.N = p.hidden; g.K = p.n_dense;
        g.A = p.dense; g.sa_m = p.ld_dense; g.sa_k = 1; g.a_rows = ids;
        g.B = p.w; g.sb_n = p.n_dense; g.sb_k = 1;
        g.bias = p.b; g.C = out; g.ldc = ldo; g.accumulate = tables ? 1 : 0; g.act = 0;
        return mi_gemm_launch(g, ws, ws_bytes, s);
    }
    return 0;
}

size_t mi_pinsage_project_bwd_workspace_bytes(const mi_item_projector* p, int64_t n) {
    if (check_projector(p, n, true) != 0) return 0;
    return bwd_ws_bytes(*p, n);
}

int mi_pinsage_project_bwd_f32(const mi_item_projector* pp, const mi_item_projector_grads* grads, int64_t n, const int64_t* ids,
                               const float* g, int64_t ldg, void* ws, size_t ws_bytes, mi_stream_t stream) {
    return project_bwd(pp, grads, nullptr, nullptr, n, ids, g, ldg, ws, ws_bytes, stream);
}

int mi_pinsage_project_bwd_lazy_f32(const mi_item_projector* pp, const mi_item_projector_grads* grads,
                                    const mi_item_projector_moments* moments, const mi_lazy_adam* lazy, int64_t n, const int64_t* ids,
                                    const float* g, int64_t ldg, void* ws, size_t ws_bytes, mi_stream_t stream) {
    return project_bwd(pp, grads, moments, lazy, n, ids, g, ldg, ws, ws_bytes, stream);
}

int mi_pinsage_project_clear_f32(const mi_item_projector* pp, const mi_item_projector_grads* grads, int64_t n, const int64_t* ids,
                                 mi_stream_t stream) {
    int bad = check_projector(pp, n, ids != nullptr);
    if (bad) return bad;
    const mi_item_projector& p = *pp;
    bad = check_grads(p, grads, false);
    if (bad) return bad;
    const int64_t n_ref = n * n_slots(p);
    if (n_ref == 0) return 0;
    const int h4 = p.hidden / 4;
    hipLaunchKernelGGL(proj_clear_kernel, dim3(grid_for(n_ref * h4)), dim3(kBlock), 0, (hipStream_t)stream, n, n_ref, h4,
                       (int)p.n_cols, ids, p.x, grad_tables(p, *grads));
    return mi_launch_status();
}

}  // extern "C"
