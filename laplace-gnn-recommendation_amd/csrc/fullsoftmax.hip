// Exact full-catalogue softmax for the LightGCN trainer (mi_full_softmax_fwd_bwd_f32; the rule is in the header): every item
// of the catalogue is a candidate of every slot.  The B x I scores are 32 x 32 score tiles (loss_tiles.hpp: the lane map, the
// k order and the rescale order that its passes share, so they see the same score bits) against the whole item table.
//   1. gather_kernel   the B user rows of final_emb become one contiguous [B, d] image; pos as int32 and the slot's L2 term
//                      beside it.  The item rows are read where they lie: rows [n_users, n_users + I) of final_emb.
//   2. stats_kernel    one wavefront per (32 user slots, item chunk): their scores against every 32-item tile of the chunk, a
//                      running maximum and sum per lane -> one (max, sum) pair per slot and chunk; the chunk that holds pos_b
//                      also leaves l[b, pos_b].
//      merge_kernel    one thread per slot: the pairs in ascending chunk order -> lse[b] and the slot's loss term
//   3. sweep_kernel    one wavefront per 32 OWNED rows, the other side's rows streaming past
//        users own    grid (user tiles, item chunks): a partial row of dL/df[users_b] per slot and chunk, then
//                      chunk_sum_kernel adds a slot's partial rows in ascending chunk order -> the slot row
//        items own     grid (item tiles): the wavefront owns its 32 item rows for the whole pass over the B users and stores
//                      them straight into g_final (item rows are unique: one writer per row); it also counts the slots that
//                      name each of its items, which is the item's reg_w
//   4. refs / sort / chunk / combine   the B slot rows become user rows of g_final: the sorted-reference segmented sum of
//                      refsum.hpp (a user may hold several slots); the users' reg_w from the run lengths
//   5. refsum::finish_kernel   loss = sum(term) / B + lambda * sum(reg), one block, fixed order
// No float atomics; every order of summation is a function of (B, I, d) and the ids — split_catalogue never asks the device
// for its size — so two calls give equal bits, here and on any other gfx950.
// This file owns the cut of the catalogue (split_catalogue), the masks and chunking of its kernels, the two chunk merges and
// the host entry.
//
// Decomposition.  A user tile streams I / 32 item tiles (3 125 at I = 100 000) and B / 32 = 512 wavefronts at B = 16 384 do
// not fill the chip's 1 024 SIMDs, where one resident wavefront hides no load behind its 64-cycle matrix instructions.  The
// catalogue is therefore cut into item chunks for the statistics and the user sweep, enough of them for kWaveTarget wavefronts
// (at most kMaxChunks, at least one tile each).  The other candidate, a workgroup of several wavefronts that interleave item
// tiles and reduce in LDS, keeps the same loads per wavefront and adds a barrier per tile; the chunk split costs B x d floats
// of workspace per chunk and two small merge kernels (18 us together at B = 16 384) instead, and was built.
// A/B of the wavefront target at B = 16 384, I = 100 000 (ms of the whole call, d = 64 / d = 128; profiles/full_softmax.md):
//   512 (one chunk) 35.96 / 65.50    1 024  23.70 / 50.88    2 048  18.65 / 37.28    4 096  16.26 / 36.88
//   8 192  16.11 / 35.01    16 384  15.86 / 33.86, whose 32 chunks of partial rows (256 MiB at d = 128) buy 3 %: 8 192 it is.
//   (The first two were taken before score_tile loaded its operand in groups, which moved the others by 0 to 5 %.)
#include "loss_tiles.hpp"
#include "refsum.hpp"

namespace {

using namespace loss_tiles;

constexpr int kLoadGroup = 4;    // k steps of a score tile whose A chunks are loaded together, a group ahead
constexpr int64_t kWaveTarget = 8192;   // wavefronts the chunked passes aim for
constexpr int64_t kMaxChunks = 32;

// The cut of the catalogue into item chunks: a function of (B, I) alone.
struct Split {
    int64_t tiles_per_chunk, chunks;
};
Split split_catalogue(int64_t batch, int64_t n_items) {
    const int64_t user_tiles = mi_ceil_div(batch, kTile), item_tiles = mi_ceil_div(n_items, kTile);
    int64_t want = mi_ceil_div(kWaveTarget, user_tiles);
    if (want > kMaxChunks) want = kMaxChunks;
    if (want > item_tiles) want = item_tiles;
    Split s;
    s.tiles_per_chunk = mi_ceil_div(item_tiles, want);
    s.chunks = mi_ceil_div(item_tiles, s.tiles_per_chunk);
    return s;
}

// ------------------------------------------------------------------ 1. gather ----------------------------------------------
// one wavefront per slot, float4 lanes
__global__ __launch_bounds__(256) void full_gather_kernel(
    int64_t batch, int d4, int64_t n_users, const int64_t* __restrict__ users, const int64_t* __restrict__ pos,
    const float4* __restrict__ fin, int64_t ldf4, const float4* __restrict__ e0, int64_t lde4, float4* __restrict__ u_img,
    int32_t* __restrict__ pid, float* __restrict__ reg_out) {
    const int64_t b = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / MI_WAVE;
    if (b >= batch) return;
    const int lane = mi_lane();
    const int64_t u = users[b], p = n_users + pos[b];
    const float4* uf = fin + u * ldf4;
    const float4* u0 = e0 + u * lde4;
    const float4* p0 = e0 + p * lde4;
    float rg = 0.f;
    for (int e = lane; e < d4; e += MI_WAVE) {
        u_img[b * d4 + e] = uf[e];
        rg = add_squares(rg, u0[e], p0[e]);
    }
    rg = mi_wave_sum(rg);
    if (lane == 0) {
        pid[b] = (int32_t)pos[b];
        reg_out[b] = rg;
    }
}

// ------------------------------------------------------------------ 2. row statistics --------------------------------------
// One wavefront per (32 user slots, item chunk): blockIdx.x the user tile, blockIdx.y the chunk; their (max, sum) over the
// chunk's item tiles, tiles ascending.  Items past the catalogue count as -inf.
__global__ __launch_bounds__(MI_WAVE) void full_stats_kernel(
    Rows users, Rows items, int d4, int nq, int64_t tiles_per_chunk, int64_t bp /* slots, whole tiles */,
    const int32_t* __restrict__ pid, float* __restrict__ part_max, float* __restrict__ part_sum,
    float* __restrict__ diag_out) {
    extern __shared__ float4 tile[];
    const int lane = mi_lane(), c = lane & 31, h = lane >> 5;
    const int64_t b0 = (int64_t)blockIdx.x * kTile, chunk = blockIdx.y;
    load_owned_tile(tile, users, b0, d4, nq);
    __syncthreads();
    const int64_t b = b0 + c;
    const int64_t my_p = pid[min(b, users.n - 1)];
    const int64_t t0 = chunk * tiles_per_chunk, t1 = min(t0 + tiles_per_chunk, (items.n + kTile - 1) / kTile);
    const float ninf = -INFINITY;
    MaxSum run;
    float diag = ninf;
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t j0 = t * kTile;
        const f32x16 acc = score_tile<kLoadGroup>(items, j0, d4, nq, tile);
        float x[16];
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4)   // registers 4 q4 + i: rows 8 q4 + 4 h + i of the tile (the lane map)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int64_t j = j0 + 8 * q4 + 4 * h + i;
                x[4 * q4 + i] = j < items.n ? acc[4 * q4 + i] : ninf;
                if (j == my_p) diag = acc[4 * q4 + i];
            }
        lse_add_tile(run, x);
    }
    const MaxSum all = lse_fold_halves(run, h);
    diag = fmaxf(diag, __shfl_xor(diag, 32, MI_WAVE));
    if (b < users.n && h == 0) {   // item 0 of the chunk's first tile is a row of half 0: the maximum is finite
        part_max[chunk * bp + b] = all.m;
        part_sum[chunk * bp + b] = all.s;
        if (diag > ninf) diag_out[b] = diag;   // pos_b lies in exactly one chunk: one writer
    }
}

// One thread per slot: the chunks' (max, sum) pairs, ascending.  One chunk and one item: exp(0) = 1, log(1) = 0, lse = l.
__global__ __launch_bounds__(256) void full_merge_kernel(int64_t batch, int64_t bp, int64_t chunks,
                                                         const float* __restrict__ part_max,
                                                         const float* __restrict__ part_sum, const float* __restrict__ diag,
                                                         float* __restrict__ lse_out, float* __restrict__ term_out) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    float mx = part_max[b];
    for (int64_t k = 1; k < chunks; ++k) mx = fmaxf(mx, part_max[k * bp + b]);
    float sum = 0.f;
    for (int64_t k = 0; k < chunks; ++k) sum += part_sum[k * bp + b] * expf(part_max[k * bp + b] - mx);
    const float lse = mx + logf(sum);
    lse_out[b] = lse;
    term_out[b] = lse - diag[b];
}

// ------------------------------------------------------------------ 3. gradient sweeps -------------------------------------
struct SweepArgs {
    Rows users, items;
    int d, nq;
    int64_t tiles_per_chunk;            // users own: the item tiles of a chunk (blockIdx.y)
    const int32_t* __restrict__ pid;    // [whole tiles of slots]
    const float* __restrict__ lse;      // [whole tiles of slots]
    float w;                            // g_scale / B
    float* __restrict__ dst;            // users own: [chunks, B, d] partial rows; items own: the item rows of g_final
    int64_t ldd;
    float* __restrict__ reg_w;          // items own: the item entries of reg_w, or null
    float reg_unit;                     // 2 * lambda * reg_scale: one reference's share
};

// kOwnUsers: the owned rows are user slots (dL/df[users_b] = sum_i c[b,i] f[n_users + i], streamed rows = the chunk's items);
// otherwise they are items (dL/df[n_users + i] = sum_b c[b,i] f[users_b], streamed rows = all B user slots).
// NT = the 32-column tiles of a row.
template <int NT, bool kOwnUsers>
__global__ __launch_bounds__(MI_WAVE) void full_sweep_kernel(SweepArgs a) {
    extern __shared__ float4 tile[];
    const int lane = mi_lane(), c = lane & 31, h = lane >> 5;
    const int d = a.d, d4 = d / 4, nq = a.nq;
    const Rows own = kOwnUsers ? a.users : a.items;
    const Rows str = kOwnUsers ? a.items : a.users;
    const int64_t o0 = (int64_t)blockIdx.x * kTile;
    load_owned_tile(tile, own, o0, d4, nq);
    __syncthreads();
    const int64_t o = o0 + c;
    const bool o_live = o < own.n;
    const int64_t str_tiles = (str.n + kTile - 1) / kTile;
    const int64_t t0 = kOwnUsers ? (int64_t)blockIdx.y * a.tiles_per_chunk : 0;
    const int64_t t1 = kOwnUsers ? min(t0 + a.tiles_per_chunk, str_tiles) : str_tiles;
    // users own: the slot's own statistics; the arrays are padded to whole tiles, and o0 + c stays inside them
    const float my_lse = kOwnUsers ? a.lse[o] : 0.f;
    const int64_t my_p = kOwnUsers ? (int64_t)a.pid[o] : 0;
    int named = 0;   // items own: the slots that name item o, over this lane half's rows
    f32x16 out[NT];
    grad_zero(out);
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t r0 = t * kTile;
        const f32x16 acc = score_tile<kLoadGroup>(str, r0, d4, nq, tile);
        f32x16 cf;
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
            const int64_t base = r0 + 8 * q4 + 4 * h;
            float lses[4] = {my_lse, my_lse, my_lse, my_lse};
            int64_t ps[4] = {my_p, my_p, my_p, my_p};
            if (!kOwnUsers) {   // the streamed rows are slots: their statistics, four at a time (whole tiles: inside the arrays)
                const float4 sr = *reinterpret_cast<const float4*>(a.lse + base);
                const int4 pr = *reinterpret_cast<const int4*>(a.pid + base);
                lses[0] = sr.x; lses[1] = sr.y; lses[2] = sr.z; lses[3] = sr.w;
                ps[0] = pr.x; ps[1] = pr.y; ps[2] = pr.z; ps[3] = pr.w;
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int64_t r = base + i;
                const int64_t item = kOwnUsers ? r : o;
                const bool hit = item == ps[i];
                const bool outside = r >= str.n || !o_live;
                const float e = expf(acc[4 * q4 + i] - lses[i]);
                cf[4 * q4 + i] = outside ? 0.f : a.w * (e - (hit ? 1.f : 0.f));
                if (!kOwnUsers) named += (!outside && hit) ? 1 : 0;
            }
        }
        grad_add_tile(out, cf, str, r0, d);
    }
    grad_store(out, a.dst + (kOwnUsers ? (int64_t)blockIdx.y * own.n * a.ldd : 0), a.ldd, o0, own.n, d);
    if (!kOwnUsers) {
        named += __shfl_xor(named, 32, MI_WAVE);
        if (a.reg_w && h == 0 && o_live && named) a.reg_w[o] = (float)named * a.reg_unit;   // reg_w is zero on entry
    }
}

// A slot's partial rows in ascending chunk order -> its slot row.  One float4 per thread.
__global__ __launch_bounds__(256) void full_chunk_sum_kernel(int64_t n4 /* B * d / 4 */, int64_t chunks,
                                                             const float4* __restrict__ part, float4* __restrict__ g_slot) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    float4 acc = part[i];
    for (int64_t k = 1; k < chunks; ++k) acc = mi_f4_add(acc, part[k * n4 + i]);
    g_slot[i] = acc;
}

// ------------------------------------------------------------------ 4. slot rows -> user rows ------------------------------
__global__ void full_refs_kernel(int64_t batch, const int64_t* __restrict__ users, uint32_t* __restrict__ keys,
                                 uint32_t* __restrict__ refs) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // reference id = the slot = its row of g_slot
    if (b >= batch) return;
    keys[b] = (uint32_t)users[b];
    refs[b] = (uint32_t)b;
}

template <int VPT>  // floats of a row per lane: ceil(d / 64)
__global__ __launch_bounds__(refsum::kBlock) void full_chunk_kernel(
    int64_t batch, const float* __restrict__ g_slot, const uint32_t* __restrict__ keys, const uint32_t* __restrict__ refs,
    refsum::Dest to, float* __restrict__ reg_w, float reg_unit) {
    const refsum::Chunk c = refsum::open_chunk(keys, batch);
    if (c.n_here == 0) return;
    refsum::SlotRow term;
    if (c.lane < c.n_here) {
        term.src = refs[c.j0 + c.lane];
        if (reg_w) {
            const int64_t len = refsum::run_length(keys, c.j0 + c.lane, batch);
            if (len) reg_w[c.key] = (float)len * reg_unit;   // the key is the user's row
        }
    }
    refsum::walk_references<VPT>(c, term, g_slot, to.d, to);
}

// ------------------------------------------------------------------ host ---------------------------------------------------
bool args_in_range(int64_t batch, int64_t d, int64_t n_items) {
    return batch >= 1 && 2 * batch < INT32_MAX && d >= 4 && d % 4 == 0 && d <= kMaxD && n_items >= 1 && n_items < INT32_MAX;
}

struct Workspace {
    float *u_img, *g_slot, *part, *lse, *term, *reg, *diag, *part_max, *part_sum;
    int32_t* pid;
    refsum::Buffers sum;   // partial rows of d floats: this entry knows its d
    bool ok() const { return u_img && g_slot && part && lse && term && reg && diag && part_max && part_sum && pid && sum.ok(); }
};

Workspace carve(MiArena& a, int64_t batch, int64_t d, int64_t chunks) {
    const size_t b = (size_t)batch, bp = (size_t)mi_ceil_div(batch, kTile) * kTile;   // id and statistic arrays: whole tiles
    Workspace w;
    w.u_img = a.take<float>(b * d);
    w.g_slot = a.take<float>(b * d);
    w.part = a.take<float>((size_t)chunks * b * d);
    w.pid = a.take<int32_t>(bp);
    w.lse = a.take<float>(bp);
    w.term = a.take<float>(bp);
    w.reg = a.take<float>(bp);
    w.diag = a.take<float>(bp);
    w.part_max = a.take<float>((size_t)chunks * bp);
    w.part_sum = a.take<float>((size_t)chunks * bp);
    w.sum = refsum::take(a, batch, d);
    return w;
}

}  // namespace

extern "C" {

size_t mi_full_softmax_workspace_bytes(int64_t batch, int64_t d, int64_t n_items) {
    if (!args_in_range(batch, d, n_items)) return 0;
    const size_t b = (size_t)batch, bp = (size_t)mi_ceil_div(batch, kTile) * kTile;
    const size_t chunks = (size_t)split_catalogue(batch, n_items).chunks;
    return 2 * mi_align_up(b * d * sizeof(float), 256) + mi_align_up(chunks * b * d * sizeof(float), 256) +
           5 * mi_align_up(bp * sizeof(float), 256) + 2 * mi_align_up(chunks * bp * sizeof(float), 256) +
           refsum::workspace_bytes(batch, d);
}

int mi_full_softmax_fwd_bwd_f32(int64_t batch, int64_t d, int64_t n_users, int64_t n_items, const int64_t* users,
                                const int64_t* pos, const float* final_emb, int64_t ldf, const float* e0, int64_t lde,
                                float lambda, float g_scale, float reg_scale, float* loss_out, float* g_final, int64_t ldg,
                                float* reg_w, void* ws, size_t ws_bytes, mi_stream_t stream) {
    MI_CHECK_ARG(batch >= 1 && d > 0 && n_users >= 0 && n_items >= 1);
    if (d % 4 != 0 || d > kMaxD) return MI_ERR_UNSUPPORTED;
    if (!g_final && reg_w) return MI_ERR_UNSUPPORTED;   // the loss-only form counts no references
    if (2 * batch >= INT32_MAX || n_items >= INT32_MAX) return MI_ERR_TOO_LARGE;
    MI_CHECK_ARG(users && pos && final_emb && e0 && loss_out && ws);
    MI_CHECK_ARG(ldf >= d && lde >= d && ldf % 4 == 0 && lde % 4 == 0 && (!g_final || ldg >= d));
    MI_CHECK_ARG(mi_aligned16(final_emb) && mi_aligned16(e0) && mi_aligned16(ws));
    MI_CHECK_ARG(((uintptr_t)users | (uintptr_t)pos) % 8 == 0);
    MI_CHECK_ARG(((uintptr_t)loss_out | (uintptr_t)g_final | (uintptr_t)reg_w) % 4 == 0);
    if (ws_bytes < mi_full_softmax_workspace_bytes(batch, d, n_items)) return MI_ERR_WORKSPACE;
    const Split cut = split_catalogue(batch, n_items);
    MiArena arena(ws, ws_bytes);
    const Workspace w = carve(arena, batch, d, cut.chunks);
    if (!w.ok()) return MI_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int64_t user_tiles = mi_ceil_div(batch, kTile), item_tiles = mi_ceil_div(n_items, kTile);
    const int64_t bp = user_tiles * kTile;
    const int d4 = (int)(d / 4), nq = (int)mi_align_up((size_t)(d4 + 1) / 2, kLoadGroup);   // k steps: whole groups
    const size_t lds = (size_t)kTile * (2 * nq + 1) * sizeof(float4);   // 33 280 bytes at d = 256
    refsum::Sort sorted;
    if (g_final) {
        const int rc = refsum::plan_sort(w.sum, batch, false, s, sorted);
        if (rc) return rc;
    }
    // ---- nothing has been enqueued up to here ----
    const Rows user_rows{reinterpret_cast<const float4*>(w.u_img), d4, batch};
    const Rows item_rows{reinterpret_cast<const float4*>(final_emb + n_users * ldf), ldf / 4, n_items};
    hipLaunchKernelGGL(full_gather_kernel, dim3((unsigned)mi_ceil_div(batch * MI_WAVE, 256)), dim3(256), 0, s, batch, d4,
                       n_users, users, pos, reinterpret_cast<const float4*>(final_emb), ldf / 4,
                       reinterpret_cast<const float4*>(e0), lde / 4, reinterpret_cast<float4*>(w.u_img), w.pid, w.reg);
    hipLaunchKernelGGL(full_stats_kernel, dim3((unsigned)user_tiles, (unsigned)cut.chunks), dim3(MI_WAVE), lds, s, user_rows,
                       item_rows, d4, nq, cut.tiles_per_chunk, bp, (const int32_t*)w.pid, w.part_max, w.part_sum, w.diag);
    hipLaunchKernelGGL(full_merge_kernel, dim3((unsigned)mi_ceil_div(batch, 256)), dim3(256), 0, s, batch, bp, cut.chunks,
                       (const float*)w.part_max, (const float*)w.part_sum, (const float*)w.diag, w.lse, w.term);
    if (g_final) {
        const float reg_unit = 2.0f * reg_scale * lambda;
        SweepArgs a;
        a.users = user_rows; a.items = item_rows; a.d = (int)d; a.nq = nq; a.tiles_per_chunk = cut.tiles_per_chunk;
        a.pid = w.pid; a.lse = w.lse; a.w = g_scale / (float)batch; a.reg_unit = reg_unit;
        SweepArgs by_user = a, by_item = a;
        by_user.dst = cut.chunks > 1 ? w.part : w.g_slot; by_user.ldd = d; by_user.reg_w = nullptr;
        by_item.dst = g_final + n_users * ldg; by_item.ldd = ldg; by_item.reg_w = reg_w ? reg_w + n_users : nullptr;
        refsum::with_vpt(mi_ceil_div(d, 32), [&](auto nt) {
            constexpr int NT = decltype(nt)::value;
            hipLaunchKernelGGL((full_sweep_kernel<NT, true>), dim3((unsigned)user_tiles, (unsigned)cut.chunks), dim3(MI_WAVE),
                               lds, s, by_user);
            hipLaunchKernelGGL((full_sweep_kernel<NT, false>), dim3((unsigned)item_tiles), dim3(MI_WAVE), lds, s, by_item);
        });
        if (cut.chunks > 1) {
            const int64_t n4 = batch * d4;
            hipLaunchKernelGGL(full_chunk_sum_kernel, dim3((unsigned)mi_ceil_div(n4, 256)), dim3(256), 0, s, n4, cut.chunks,
                               reinterpret_cast<const float4*>(w.part), reinterpret_cast<float4*>(w.g_slot));
        }
        hipLaunchKernelGGL(full_refs_kernel, dim3((unsigned)mi_ceil_div(batch, 256)), dim3(256), 0, s, batch, users, w.sum.k0,
                           w.sum.r0);
        const int rc = refsum::sort(w.sum, batch, s, sorted);
        if (rc) return rc;
        const refsum::Dest to{g_final, ldg, w.sum.part_head, w.sum.part_tail, (int)d};
        refsum::with_vpt(mi_ceil_div(d, MI_WAVE), [&](auto vpt) {
            constexpr int V = decltype(vpt)::value < 4 ? decltype(vpt)::value : 4;   // d <= 256
            hipLaunchKernelGGL(full_chunk_kernel<V>, refsum::chunk_grid(batch), dim3(refsum::kBlock), 0, s, batch,
                               (const float*)w.g_slot, (const uint32_t*)sorted.keys.current(),
                               (const uint32_t*)sorted.refs.current(), to, reg_w, reg_unit);
            refsum::launch_combine<V>(sorted, batch, to, s);
        });
    }
    refsum::launch_finish(batch, w.term, w.reg, 1.0f / (float)batch, lambda, loss_out, s);
    return mi_launch_status();
}

}  // extern "C"
