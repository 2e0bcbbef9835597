// Implicit ALS, block row solver (include/laplace_hip.h "iALS block", additive to ABI 14): a row-local iALS++ (Rendle et al.,
// RecSys 2021).  Instead of one d x d system per row (csrc/als.hip) a row's quadratic is minimised exactly over one block of
// B coordinates at a time: the largest system on chip is B x B, the width goes to 256, and a short row costs about
// 2 n d B + 2 d^2 + d B^2 / 3 flop per sweep instead of 2 n d^2 + d^3 / 3.  The numerics (the order of every sum) are the
// header's rule; this comment is about the layout.
//
// One WAVEFRONT per row, four rows per workgroup, no workgroup barrier anywhere: everything a row needs is private to its
// wavefront (its quarter of the LDS), so a step of the small factorisation costs a wavefront-scope fence instead of a
// barrier with three other wavefronts waiting on it, and four short rows share a workgroup.  A hub row is walked by its
// one wavefront (profiles/als_block.md has the tail that causes).
//
// Factor rows.  A row of at most R = mi_als_block_chunk(d, B) entries is RESIDENT: its factor rows are gathered once, with
// 16-byte loads, into the wavefront's 16 KiB area as [entry][LDR] floats, and its predictions p_e live in LDS.  A longer row
// STREAMS: per block it re-gathers the block's B columns of KT entries at a time (64-byte pieces of a row at B = 16) into the
// same area as [entry][LDB], once for the Gram pass and once for the prediction update, and keeps p_e in the workspace at
// the entry's position in idx.  Both forms run the same arithmetic in the same order, so the bits do not depend on which one
// a row took.  LDR and LDB are 16 mod 32 floats: the 16 columns x 2 entries that a half-wave of a ds_read_b32 touches fall
// on 32 different banks.
//
// Block step.  v_mfma_f32_16x16x4_f32 takes A[i = lane & 15][k = lane >> 4] and B[k = lane >> 4][j = lane & 15].  With the
// ENTRIES as k, the operand of tile row ti is one ds_read_b32 (column 16 ti + i of entry 4 step + k) and serves as A of the
// tiles (ti, .) and as B of the tiles (., ti): the lower-triangle tiles of the block Gram (1, 3 or 10 at B = 16, 32, 64) are
// one fmaf chain over the row's entries each.  The gradient's sum_e w_e y_e[j] rides on the same instruction: the B operand
// is w_e for every column, so every column of the result tile holds the sum.  q = G[pi, :] x is B x (64 / B) lanes of
// partial chains over rows of G with 16-byte loads from L2: a first small kernel writes G(j, k) = G[max][min] out as a full
// matrix into the workspace, so that a row of it is contiguous (the caller's upper triangle is never read).  The B x B
// Cholesky runs in the wavefront's LDS, lanes as a B x (64 / B) grid over (row, column group), the right-hand side carried in
// one register per lane (forward substitution inside the factorisation's step, x_k handed round by a lane shuffle, as the
// backward substitution).
//
// Hub rows ("iALS block hub" in the header; the mi_als_block_rows_hub entries only).  A row with more than hub_threshold
// entries is not walked by a wavefront: its d x d system is formed ONCE, over several workgroups, and the block steps run on
// that.  Four launches in front of the block kernel, on the same stream:
//   plan      one thread per work row; a hub row takes a row slot and one chunk slot per L_h = mi_als_block_hub_chunk(d) of its
//             entries (integer atomics on two counters: WHICH slot may differ from run to run, what is written there does not).
//   partial   one workgroup per chunk slot: (S_c, s_c) by csrc/als_gram.hpp — the Cholesky solver's gather / MFMA loop, with a
//             DP = 256 width class beside its four (136 lower-triangle tiles, 34 accumulator tiles per wavefront; 34 KiB of
//             staging, 68 KiB weighted).  A slot holds the lower-triangle tiles in the MFMA's C layout (tile q = ti (ti + 1) / 2
//             + tj at q * 256 + reg * 64 + lane) and s behind them.
//   assemble  grid (row slot, tile): thread (reg, lane) of tile q owns ONE element, adds its chunks in ascending c, forms A by
//             the system line and writes A[j][k] and A[k][j] into the row's full matrix (a row of it is contiguous); the last
//             grid column does s and b.  One owner and one chain per element however many workgroups a row has.
//   solve     one wavefront per hub row: u = A[pi, :] x with 16-byte loads of A from L2 in the chain layout of q above,
//             H = A[pi, pi] to LDS, the same B x B Cholesky (ab_chol_solve), x += delta.  No p_e, no entries.
// The block kernel then leaves a row with more than hub_threshold entries alone when it has a slot, and zeroes and counts it
// when it has none (the caller's hub counts were too small).  The old entries pass no threshold and no slot array.
#include "common.hpp"
#include "als_gram.hpp"

namespace {

constexpr int AB_WAVES = 4;      // rows per workgroup, one wavefront each
constexpr int AB_AREA = 4096;     // floats of LDS per wavefront for factor rows
constexpr int AB_MAX_D = 256;
constexpr int AB_MAX_RES = 256;   // entries of p_e kept in LDS
constexpr int AB_MAX_RES_W = 128;  // weighted: entries of p_e and of a_e kept in LDS, together the size of the unweighted p_e

// the smallest stride >= w that is 16 mod 32
__host__ __device__ constexpr int ab_ld(int w) { return (w + 15) / 32 * 32 + 16; }
__host__ __device__ constexpr int ab_res_of(int d) {
    return (AB_AREA / ab_ld(d) & ~3) < AB_MAX_RES ? (AB_AREA / ab_ld(d) & ~3) : AB_MAX_RES;
}

struct AbArgs {
    int n_rows, d, n_cols, n_work, nnz, sweeps, from_zero;
    const int32_t* ptr;
    const int32_t* idx;
    const float* Y;
    int64_t ldy;
    float alpha, reg;
    float* X;
    int64_t ldx;
    const int32_t* row_list;
    int32_t* n_failed;
    float* Gs;   // workspace: G(j, k) as a full symmetric matrix
    float* pw;   // workspace: p_e of the streaming rows, by entry position
    const float* conf;       // weighted entry only: a_e by entry position
    const float* reg_rows;   // weighted entry only: reg by ROW ID, or null (the scalar reg)
    int hub_thr;               // a row with more entries is a hub row; AB_NO_HUB: there are none
    const int32_t* hub_slot;   // hub entries only: [n_work] the row slot of a hub row, -1 = it found none
};

constexpr int AB_NO_HUB = 0x7fffffff;

__global__ void als_block_sym_kernel(const float* G, float* Gs, int d) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d * d) return;
    const int j = i / d, k = i - j * d;
    Gs[i] = G[k <= j ? j * d + k : k * d + j];
}

// What one lane wrote (LDS, or the row's own workspace entries) is read by the other lanes of ITS wavefront behind this.
__device__ __forceinline__ void ab_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Entries [q0, q0 + cnt) of idx, columns [col0, col0 + 4 W4) of their factor rows, to dst[e][ld]; columns at or beyond d,
// entries with an id outside the table and the entries from cnt up to the next multiple of 4 are staged as zeros.
__device__ __forceinline__ void ab_gather(const AbArgs& a, int q0, int cnt, int col0, int W4, float* dst, int ld) {
    const int lane = mi_lane();
    const int slots = ((cnt + 3) & ~3) * W4;
    for (int f = lane; f < slots; f += MI_WAVE) {
        const int e = f / W4, c4 = f - e * W4;
        float4 v = mi_f4_zero();
        if (e < cnt && col0 + 4 * c4 < a.d) {
            const int col = a.idx[q0 + e];
            if ((unsigned)col < (unsigned)a.n_cols) v = *reinterpret_cast<const float4*>(a.Y + (int64_t)col * a.ldy + col0 + 4 * c4);
        }
        *reinterpret_cast<float4*>(dst + e * ld + 4 * c4) = v;
    }
}

// t_e = sum over the first 16 nt columns of src[e][.] * vec[.] for the staged entries e < cnt: 16 lanes per entry, lane c a
// chain over columns c, c + 16, ..; the 16 chains added pairwise at lane distances 8, 4, 2, 1.  sink(e, t_e) on one lane.
template <class F>
__device__ __forceinline__ void ab_dots(const float* src, int ld, int cnt, const float* vec, int nt, F&& sink) {
    const int lane = mi_lane(), c = lane & 15;
    for (int e4 = 0; e4 < cnt; e4 += 4) {
        const int e = e4 + (lane >> 4);
        float tsum = 0.f;
        for (int i = 0; i < nt; ++i) tsum = fmaf(src[e * ld + c + 16 * i], vec[c + 16 * i], tsum);
        tsum += __shfl_xor(tsum, 8, MI_WAVE);
        tsum += __shfl_xor(tsum, 4, MI_WAVE);
        tsum += __shfl_xor(tsum, 2, MI_WAVE);
        tsum += __shfl_xor(tsum, 1, MI_WAVE);
        if (c == 0 && e < cnt) sink(e, tsum);
    }
}

// H delta = v for the bw x bw system whose lower triangle is Hs[row][HB] in the wavefront's LDS; lane l < bw brings element l of
// the right-hand side in v and leaves with delta[l].  A right-looking Cholesky, lane (i, jg) updates row i's columns
// k + 1 + jg, + JG, ..; the right-hand side goes through the forward substitution inside the factorisation's step and through
// the backward one by lane shuffles.  false at a pivot that is not a positive finite number (every lane reads the same word).
template <int B>
__device__ __forceinline__ bool ab_chol_solve(float* Hs, int bw, float& v) {
    constexpr int JG = 64 / B, HB = B + 1;
    const int lane = mi_lane(), i = lane & (B - 1), jg = lane / B;
    float myinv = 0.f;
    for (int k = 0; k < bw; ++k) {
        const float pv = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(Hs[k * HB + k])));
        if (!(pv > 0.f && pv < INFINITY)) return false;
        const float inv = 1.0f / sqrtf(pv);
        if (lane == k) myinv = inv;
        const bool below = i > k && i < bw;
        const float li = below ? Hs[i * HB + k] * inv : 0.f;
        const float yk = __shfl(v, k, MI_WAVE) * inv;
        if (lane == k) v = yk;
        else if (lane > k && lane < bw) v = fmaf(-li, yk, v);
        if (below) {   // four columns at a time: their eight LDS reads are in flight together
            for (int jb = k + 1 + jg; jb <= i; jb += 4 * JG) {
                float lj[4], h[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int jc = jb + u * JG;
                    lj[u] = jc <= i ? Hs[jc * HB + k] : 0.f;
                    h[u] = jc <= i ? Hs[i * HB + jc] : 0.f;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int jc = jb + u * JG;
                    if (jc <= i) Hs[i * HB + jc] = fmaf(-li, lj[u] * inv, h[u]);
                }
            }
        }
        if (below && jg == 0) Hs[i * HB + k] = li;
        ab_wave_sync();
    }
    for (int k = bw - 1; k >= 0; --k) {
        const float dk = __shfl(v * myinv, k, MI_WAVE);
        if (lane == k) v = dk;
        else if (lane < k) v = fmaf(-Hs[k * HB + lane], dk, v);
    }
    return true;
}

// W: the weighted entry ("iALS block weighted" in the header).  a_e sits beside p_e: in LDS (as[e]) for a resident row, re-read
// from conf with every streamed chunk otherwise, never copied into the workspace.  The B operand of the Gram tiles is
// z_e = a_e * y_e, one f32 product made in registers from the operand that the A side reads: no second staged image.
// p_e and a_e share the LDS that p_e alone has in the unweighted kernel (two workgroups per CU at B = 16 either way), so a
// weighted row is resident up to min(R, AB_MAX_RES_W) entries: fewer than R only at d <= 16.
template <int B, bool W>
__global__ __launch_bounds__(AB_WAVES * MI_WAVE) void als_block_kernel(AbArgs a) {
    constexpr int TB = B / 16, JG = 64 / B, HB = B + 1;
    constexpr int LDB = ab_ld(B), KT = B == 64 ? 48 : 64;
    static_assert(KT * LDB <= AB_AREA && KT % 4 == 0, "a streamed chunk fits the area");
    __shared__ __align__(16) float s_area[AB_WAVES][AB_AREA];
    __shared__ float s_h[AB_WAVES][B * HB];
    __shared__ __align__(16) float s_x[AB_WAVES][AB_MAX_D];
    __shared__ float s_p[AB_WAVES][W ? AB_MAX_RES_W : AB_MAX_RES];
    __shared__ float s_dl[AB_WAVES][64];
    __shared__ float s_gt[AB_WAVES][64];
    const int wave = threadIdx.x >> 6, lane = mi_lane();
    const int pos = blockIdx.x * AB_WAVES + wave;
    if (pos >= a.n_work) return;
    float* area = s_area[wave];
    float* Hs = s_h[wave];
    float* xs = s_x[wave];
    float* ps = s_p[wave];
    float* dl = s_dl[wave];
    float* gt = s_gt[wave];
    float* as = nullptr;
    if constexpr (W) {
        __shared__ float s_a[AB_WAVES][AB_MAX_RES_W];
        as = s_a[wave];
    }
    const int d = a.d, LDR = ab_ld(d), RES = W ? min(ab_res_of(d), AB_MAX_RES_W) : ab_res_of(d), d16 = (d + 15) & ~15;
    const int r = a.row_list ? a.row_list[pos] : pos;
    float* xout = a.X + (int64_t)pos * a.ldx;
    int p0 = 0, n = 0;
    if ((unsigned)r < (unsigned)a.n_rows) {
        p0 = a.ptr[r];
        n = a.ptr[r + 1] - p0;
    }
    if (n <= 0) {
        for (int k = lane; k < d; k += MI_WAVE) xout[k] = 0.f;
        return;
    }
    const bool hub = n > a.hub_thr;
    if (hub && a.hub_slot[pos] >= 0) return;   // solved from its assembled system: not this kernel's row
    // a rowptr that disagrees with nnz: nothing of idx is read for this row.  A hub row without a slot is a failed row too.
    bool failed = hub || p0 < 0 || n > a.nnz - p0;
    const bool resident = n <= RES;
    const float c1 = -(1.0f + a.alpha);
    float reg_r = a.reg;
    if constexpr (W) {
        if (a.reg_rows) reg_r = a.reg_rows[r];   // by row id; r is inside [0, n_rows) here
        failed = failed || !(reg_r > 0.f && reg_r < INFINITY);
    }
    if (!failed) {
        for (int k = lane; k < d16; k += MI_WAVE) xs[k] = (k < d && !a.from_zero) ? xout[k] : 0.f;
        if (resident) ab_gather(a, p0, n, 0, LDR / 4, area, LDR);
        if constexpr (W) {
            if (resident) {
                for (int e = lane; e < n; e += MI_WAVE) as[e] = a.conf[p0 + e];
            }
        }
        ab_wave_sync();
        // p_e = y_e . x
        if (a.from_zero) {
            for (int e = lane; e < n; e += MI_WAVE) {
                if (resident) ps[e] = 0.f; else a.pw[p0 + e] = 0.f;
            }
        } else if (resident) {
            ab_dots(area, LDR, n, xs, d16 / 16, [&](int e, float v) { ps[e] = v; });
        } else {
            for (int c0 = 0; c0 < n; c0 += RES) {
                const int cnt = min(RES, n - c0);
                ab_gather(a, p0 + c0, cnt, 0, LDR / 4, area, LDR);
                ab_wave_sync();
                ab_dots(area, LDR, cnt, xs, d16 / 16, [&](int e, float v) { ps[e] = v; });
                ab_wave_sync();
                for (int e = lane; e < cnt; e += MI_WAVE) a.pw[p0 + c0 + e] = ps[e];
                ab_wave_sync();
            }
        }
        ab_wave_sync();
    }
    const int nblk = (d + B - 1) / B;
    const int arow = lane >> 4, acol = lane & 15;
    for (int t = 0; t < a.sweeps && !failed; ++t) {
        for (int c = 0; c < nblk && !failed; ++c) {
            const int cB = c * B, bw = min(B, d - cB), bt = (bw + 15) >> 4;
            // the block's own part of G, in the C layout of the tiles: in flight under everything up to the Gram pass
            f32x4 gb[TB][TB];
#pragma unroll
            for (int ti = 0; ti < TB; ++ti) {
#pragma unroll
                for (int tj = 0; tj <= ti; ++tj) {
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int row = 16 * ti + 4 * arow + g, col = 16 * tj + acol;
                        gb[ti][tj][g] = (row < bw && col <= row) ? a.Gs[(cB + row) * d + cB + col] : 0.f;
                    }
                }
            }
            // q[j] = sum_k G(j, k) x[k]: lane (j, kg) takes the groups of four columns kg, kg + JG, .. as one chain; the JG
            // chains are added in ascending kg
            const int j = lane & (B - 1), kg = lane / B;
            float qv = 0.f;
            if (j < bw) {
                const float4* grow = reinterpret_cast<const float4*>(a.Gs + (cB + j) * d);
                const float4* x4 = reinterpret_cast<const float4*>(xs);
#pragma unroll 8
                for (int k4 = kg; k4 < d / 4; k4 += JG) {
                    const float4 gv = grow[k4], xv = x4[k4];
                    qv = fmaf(gv.x, xv.x, qv);
                    qv = fmaf(gv.y, xv.y, qv);
                    qv = fmaf(gv.z, xv.z, qv);
                    qv = fmaf(gv.w, xv.w, qv);
                }
            }
            float q = __shfl(qv, j, MI_WAVE);
#pragma unroll
            for (int g = 1; g < JG; ++g) q += __shfl(qv, j + B * g, MI_WAVE);
            // the block Gram and sum_e w_e y_e[j], the entries as k of the matrix instruction
            f32x4 acc[TB][TB], gacc[TB];
#pragma unroll
            for (int ti = 0; ti < TB; ++ti) {
                gacc[ti] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int tj = 0; tj < TB; ++tj) acc[ti][tj] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
            auto gram = [&](const float* src, int ld, int col0, int cnt) {   // p_e of the staged entries is ps[e]
                for (int e4 = 0; e4 < cnt; e4 += 4) {
                    const int e = e4 + arow;
                    float w = 0.f, ae = 0.f;
                    if constexpr (W) {
                        if (e < cnt) {
                            ae = as[e];
                            w = fmaf(ae, ps[e], -(1.0f + ae));
                        }
                    } else {
                        if (e < cnt) w = fmaf(a.alpha, ps[e], c1);
                    }
                    float op[TB];
#pragma unroll
                    for (int ti = 0; ti < TB; ++ti) op[ti] = ti < bt ? src[e * ld + col0 + 16 * ti + acol] : 0.f;
                    float oz[TB];
#pragma unroll
                    for (int ti = 0; ti < TB; ++ti) oz[ti] = W ? ae * op[ti] : op[ti];
#pragma unroll
                    for (int ti = 0; ti < TB; ++ti) {
                        if (ti < bt) {
#pragma unroll
                            for (int tj = 0; tj <= ti; ++tj)
                                acc[ti][tj] = __builtin_amdgcn_mfma_f32_16x16x4f32(op[ti], oz[tj], acc[ti][tj], 0, 0, 0);
                            gacc[ti] = __builtin_amdgcn_mfma_f32_16x16x4f32(op[ti], w, gacc[ti], 0, 0, 0);
                        }
                    }
                }
            };
            if (resident) {
                gram(area, LDR, cB, n);
            } else {
                for (int c0 = 0; c0 < n; c0 += KT) {
                    const int cnt = min(KT, n - c0);
                    ab_gather(a, p0 + c0, cnt, cB, B / 4, area, LDB);
                    if (lane < cnt) ps[lane] = a.pw[p0 + c0 + lane];
                    if constexpr (W) {
                        if (lane < cnt) as[lane] = a.conf[p0 + c0 + lane];
                    }
                    ab_wave_sync();
                    gram(area, LDB, 0, cnt);
                    ab_wave_sync();
                }
            }
            // H = fmaf(alpha, S, G) + reg I (lower triangle) and the gradient, to LDS; weighted: H = (G + S) + reg_r I
#pragma unroll
            for (int ti = 0; ti < TB; ++ti) {
                if (ti >= bt) continue;
#pragma unroll
                for (int tj = 0; tj <= ti; ++tj) {
                    const int col = 16 * tj + acol;
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int row = 16 * ti + 4 * arow + g;
                        if (row < bw && col <= row) {
                            float v;
                            if constexpr (W) v = gb[ti][tj][g] + acc[ti][tj][g];
                            else v = fmaf(a.alpha, acc[ti][tj][g], gb[ti][tj][g]);
                            if (row == col) v = v + reg_r;
                            Hs[row * HB + col] = v;
                        }
                    }
                }
                if (acol == 0) {
#pragma unroll
                    for (int g = 0; g < 4; ++g) gt[16 * ti + 4 * arow + g] = gacc[ti][g];
                }
            }
            ab_wave_sync();
            // H delta = -g; lane l < bw carries element l of the right-hand side
            float v = lane < bw ? -fmaf(reg_r, xs[cB + lane], gt[lane] + q) : 0.f;
            if (!ab_chol_solve<B>(Hs, bw, v)) {
                failed = true;   // the same answer for every lane: the whole wavefront leaves here
                break;
            }
            if (lane < bw) xs[cB + lane] = xs[cB + lane] + v;
            dl[lane] = lane < bw ? v : 0.f;
            ab_wave_sync();
            if (t == a.sweeps - 1 && c == nblk - 1) break;   // nobody reads the predictions after the last step
            // p_e += sum_{j in pi} y_e[j] delta[j]
            if (resident) {
                ab_dots(area + cB, LDR, n, dl, bt, [&](int e, float s) { ps[e] = ps[e] + s; });
            } else {
                for (int c0 = 0; c0 < n; c0 += KT) {
                    const int cnt = min(KT, n - c0);
                    ab_gather(a, p0 + c0, cnt, cB, B / 4, area, LDB);
                    if (lane < cnt) ps[lane] = a.pw[p0 + c0 + lane];
                    ab_wave_sync();
                    ab_dots(area, LDB, cnt, dl, bt, [&](int e, float s) { ps[e] = ps[e] + s; });
                    ab_wave_sync();
                    if (lane < cnt) a.pw[p0 + c0 + lane] = ps[lane];
                    ab_wave_sync();
                }
            }
            ab_wave_sync();
        }
    }
    if (failed) {
        for (int k = lane; k < d; k += MI_WAVE) xout[k] = 0.f;
        if (lane == 0) atomicAdd(a.n_failed, 1);
        return;
    }
    for (int k = lane; k < d; k += MI_WAVE) xout[k] = xs[k];
}

// ---- hub rows ---------------------------------------------------------------------------------------------------------------

// L_h: 256 entries up to d = 64, 512 beyond.  A chunk slot (DP^2 / 2 floats, DP the width class) is then at most a quarter of
// the bytes the chunk gathers, written once and read once beside a loop that is bound by its matrix instructions, and a row
// of half a million entries is 1 036 workgroups at d = 256.  The reason for chunks this short is accuracy: a hub row's
// answer is as good as its Gram (there is no p_e to refine it, as the block rule has), and the error of a chain grows with
// its length.  On a row of L_h + 1 entries at d = 256 (warm start, three sweeps) the float32 statement of the rule was 8.4
// times as far from float64 as the float32 block reference with L_h = 2 048 and 7.9 times with 1 024, against the 8 the
// tests allow (profiles/als_hub.md).
__host__ __device__ constexpr int abh_chunk_of(int d) { return d <= 64 ? 256 : 512; }
__host__ __device__ constexpr int abh_tiles_of(int d) { return ((d + 15) / 16) * ((d + 15) / 16 + 1) / 2; }
// floats of one chunk slot: the lower-triangle tiles of S_c, then s_c
__host__ __device__ constexpr int abh_slot_of(int d) { return abh_tiles_of(d) * 256 + (d + 15) / 16 * 16; }

struct AbHub {
    int L, cap_rows, cap_chunks;
    int32_t* counters;    // [0] row slots handed out, [1] chunk slots handed out
    int32_t* slot_of;     // [n_work]  work position -> row slot, -1 = no hub row, or none left
    int32_t* row_pos;     // [cap_rows]  row slot -> work position, -1 = unused
    int32_t* row_base;    // [cap_rows]  first chunk slot of the row
    int32_t* chunk_row;   // [cap_chunks]  chunk slot -> row slot, -1 = unused
    float* part;          // [cap_chunks][abh_slot_of(d)]
    float* sys;           // [cap_rows][d * d + d]: A as a full symmetric matrix, then b
};

__global__ void abh_plan_kernel(AbArgs a, AbHub h) {
    const int pos = blockIdx.x * blockDim.x + threadIdx.x;
    if (pos >= a.n_work) return;
    const int r = a.row_list ? a.row_list[pos] : pos;
    int slot = -1;
    if ((unsigned)r < (unsigned)a.n_rows) {
        const int q0 = a.ptr[r], n = a.ptr[r + 1] - q0;
        if (n > a.hub_thr && q0 >= 0 && n <= a.nnz - q0) {
            const int nch = (n + h.L - 1) / h.L;
            const int s = atomicAdd(&h.counters[0], 1);
            const int b = (s >= 0 && s < h.cap_rows) ? atomicAdd(&h.counters[1], nch) : -1;   // no chunks for a row without a slot
            if (b >= 0 && b <= h.cap_chunks - nch) {
                slot = s;
                h.row_pos[s] = pos;
                h.row_base[s] = b;
                for (int c = 0; c < nch; ++c) h.chunk_row[b + c] = s;
            }
        }
    }
    h.slot_of[pos] = slot;
}

template <class C, bool W>
__global__ __launch_bounds__(C::NT) void abh_partial_kernel(AbArgs a, AbHub h) {
    __shared__ __align__(16) float sm[(W ? 2 : 1) * ALS_KT * C::LDA];
    const int slot = blockIdx.x;
    const int hr = h.chunk_row[slot];
    if (hr < 0) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int d = a.d;
    const int pos = h.row_pos[hr];
    const int r = a.row_list ? a.row_list[pos] : pos;
    const int c = slot - h.row_base[hr];
    const int p0 = a.ptr[r] + c * h.L, p1 = min(p0 + h.L, a.ptr[r + 1]);
    int ti[C::TPW], tj[C::TPW];
    bool live[C::TPW];
    f32x4 acc[C::TPW];
    als_tiles<C>(d, ti, tj, live);
#pragma unroll
    for (int s = 0; s < C::TPW; ++s) acc[s] = f32x4{0.f, 0.f, 0.f, 0.f};
    float s_sum = 0.f;
    if constexpr (W) {
        __shared__ float cs[ALS_KT];
        als_accumulate_w<C>(a, p0, p1, sm, cs, ti, tj, live, acc, s_sum);
    } else {
        als_accumulate<C>(a, p0, p1, sm, ti, tj, live, acc, s_sum);
    }
    float* out = h.part + (int64_t)slot * abh_slot_of(d);
#pragma unroll
    for (int s = 0; s < C::TPW; ++s) {
        if (!live[s]) continue;   // live: 16 ti < d, i.e. tile q = wave + WAVES s is one of the abh_tiles_of(d)
        float* tile = out + (wave + C::WAVES * s) * 256 + lane;
#pragma unroll
        for (int g = 0; g < 4; ++g) tile[64 * g] = acc[s][g];
    }
    if (tid < d) out[abh_tiles_of(d) * 256 + tid] = s_sum;
}

template <bool W>
__global__ __launch_bounds__(256) void abh_assemble_kernel(AbArgs a, AbHub h) {
    const int hr = blockIdx.x;
    const int pos = h.row_pos[hr];
    if (pos < 0) return;
    const int tid = threadIdx.x, d = a.d, ntl = abh_tiles_of(d), pt = abh_slot_of(d);
    const int r = a.row_list ? a.row_list[pos] : pos;
    const int nch = (a.ptr[r + 1] - a.ptr[r] + h.L - 1) / h.L;
    const float* part = h.part + (int64_t)h.row_base[hr] * pt;
    float* sys = h.sys + (int64_t)hr * (d * d + d);
    const int q = blockIdx.y;
    if (q < ntl) {
        const float* p = part + q * 256 + tid;
        float S = p[0];
#pragma unroll 8
        for (int c = 1; c < nch; ++c) S = S + p[(int64_t)c * pt];
        int ti, tj;
        als_tile_of(q, ti, tj);
        const int lane = tid & 63, g = tid >> 6;
        const int row = 16 * ti + 4 * (lane >> 4) + g, col = 16 * tj + (lane & 15);
        if (row < d && col <= row) {
            float v;
            if constexpr (W) v = a.Gs[row * d + col] + S;
            else v = fmaf(a.alpha, S, a.Gs[row * d + col]);
            if (row == col) {
                float reg_r = a.reg;
                if constexpr (W) {
                    if (a.reg_rows) reg_r = a.reg_rows[r];
                }
                v = v + reg_r;
            }
            sys[row * d + col] = v;
            sys[col * d + row] = v;
        }
    } else {
        for (int j = tid; j < d; j += 256) {
            const float* p = part + ntl * 256 + j;
            float s = p[0];
            for (int c = 1; c < nch; ++c) s = s + p[(int64_t)c * pt];
            sys[d * d + j] = W ? s : (1.0f + a.alpha) * s;
        }
    }
}

// One wavefront per hub row: the block steps on the assembled (A, b).
template <int B, bool W>
__global__ __launch_bounds__(MI_WAVE) void abh_solve_kernel(AbArgs a, AbHub h) {
    constexpr int JG = 64 / B, HB = B + 1;
    __shared__ float Hs[B * HB];
    __shared__ __align__(16) float xs[AB_MAX_D];
    const int hr = blockIdx.x, lane = mi_lane();
    const int pos = h.row_pos[hr];
    if (pos < 0) return;
    const int d = a.d;
    const int r = a.row_list ? a.row_list[pos] : pos;
    float* xout = a.X + (int64_t)pos * a.ldx;
    bool failed = false;
    if constexpr (W) {
        const float reg_r = a.reg_rows ? a.reg_rows[r] : a.reg;
        failed = !(reg_r > 0.f && reg_r < INFINITY);
    }
    const float* A = h.sys + (int64_t)hr * (d * d + d);
    const float* b = A + d * d;
    for (int k = lane; k < d; k += MI_WAVE) xs[k] = a.from_zero ? 0.f : xout[k];
    ab_wave_sync();
    const int nblk = (d + B - 1) / B;
    const int j = lane & (B - 1), kg = lane / B;
    for (int t = 0; t < a.sweeps && !failed; ++t) {
        for (int c = 0; c < nblk; ++c) {
            const int cB = c * B, bw = min(B, d - cB);
            // u[j] = sum_k A(j, k) x[k]: the chains of the block kernel's q
            float uv = 0.f;
            if (j < bw) {
                const float4* arow = reinterpret_cast<const float4*>(A + (cB + j) * d);
                const float4* x4 = reinterpret_cast<const float4*>(xs);
#pragma unroll 8
                for (int k4 = kg; k4 < d / 4; k4 += JG) {
                    const float4 av = arow[k4], xv = x4[k4];
                    uv = fmaf(av.x, xv.x, uv);
                    uv = fmaf(av.y, xv.y, uv);
                    uv = fmaf(av.z, xv.z, uv);
                    uv = fmaf(av.w, xv.w, uv);
                }
            }
            float u = __shfl(uv, j, MI_WAVE);
#pragma unroll
            for (int g = 1; g < JG; ++g) u += __shfl(uv, j + B * g, MI_WAVE);
            for (int e = lane; e < bw * bw; e += MI_WAVE) {
                const int row = e / bw, col = e - row * bw;
                if (col <= row) Hs[row * HB + col] = A[(cB + row) * d + cB + col];
            }
            ab_wave_sync();
            float v = lane < bw ? -(u - b[cB + lane]) : 0.f;
            if (!ab_chol_solve<B>(Hs, bw, v)) {
                failed = true;
                break;
            }
            if (lane < bw) xs[cB + lane] = xs[cB + lane] + v;
            ab_wave_sync();
        }
    }
    if (failed) {
        for (int k = lane; k < d; k += MI_WAVE) xout[k] = 0.f;
        if (lane == 0) atomicAdd(a.n_failed, 1);
        return;
    }
    for (int k = lane; k < d; k += MI_WAVE) xout[k] = xs[k];
}

inline bool ab_shape_ok(int64_t d, int64_t block) {
    return d >= 4 && d <= AB_MAX_D && d % 4 == 0 && (block == 16 || block == 32 || block == 64);
}

inline size_t ab_ws_g(int64_t d) { return mi_align_up((size_t)(d * d) * 4, 256); }
inline size_t ab_ws_bytes(int64_t nnz, int64_t d) { return ab_ws_g(d) + mi_align_up((size_t)(nnz > 0 ? nnz : 1) * 4, 256); }

// The hub entries' workspace: the block entry's, then the plan's integers, the chunk slots and the assembled systems.
struct AbHubLayout {
    size_t counters, slot_of, row_pos, row_base, chunk_row, part, sys, total;
};
inline AbHubLayout abh_layout(int64_t n_work, int64_t nnz, int64_t d, int64_t hub_rows, int64_t hub_chunks) {
    AbHubLayout l;
    l.counters = ab_ws_bytes(nnz, d);
    l.slot_of = l.counters + 256;
    l.row_pos = l.slot_of + mi_align_up((size_t)n_work * 4, 256);
    l.row_base = l.row_pos + mi_align_up((size_t)hub_rows * 4, 256);
    l.chunk_row = l.row_base + mi_align_up((size_t)hub_rows * 4, 256);
    l.part = l.chunk_row + mi_align_up((size_t)hub_chunks * 4, 256);
    l.sys = l.part + mi_align_up((size_t)hub_chunks * (size_t)abh_slot_of((int)d) * 4, 256);
    l.total = l.sys + mi_align_up((size_t)hub_rows * (size_t)(d * d + d) * 4, 256);
    return l;
}

inline bool abh_counts_ok(int64_t hub_threshold, int64_t hub_rows, int64_t hub_chunks) {
    const int64_t lim = (int64_t)1 << 31;
    return hub_threshold >= 1 && hub_threshold < lim && hub_rows >= 0 && hub_rows < lim && hub_chunks >= 0 && hub_chunks < lim;
}

template <class C, bool W>
void abh_launch_partial(const AbArgs& a, const AbHub& h, hipStream_t st) {
    hipLaunchKernelGGL((abh_partial_kernel<C, W>), dim3((unsigned)h.cap_chunks), dim3(C::NT), 0, st, a, h);
}

// plan, partial Grams, assembly and block steps of the hub rows, in front of the block kernel on the same stream
template <bool W>
int abh_run(const AbArgs& a, const AbHub& h, int64_t block, hipStream_t st) {
    MI_HIP(hipMemsetAsync(h.counters, 0, 256, st));
    if (h.cap_rows > 0) MI_HIP(hipMemsetAsync(h.row_pos, 0xFF, (size_t)h.cap_rows * 4, st));
    if (h.cap_chunks > 0) MI_HIP(hipMemsetAsync(h.chunk_row, 0xFF, (size_t)h.cap_chunks * 4, st));
    hipLaunchKernelGGL(abh_plan_kernel, dim3((unsigned)mi_ceil_div(a.n_work, 256)), dim3(256), 0, st, a, h);
    MI_HIP(hipGetLastError());
    if (h.cap_rows == 0 || h.cap_chunks == 0) return 0;   // no row can have a slot
    if (a.d <= 16) abh_launch_partial<AlsCfg<16, 1>, W>(a, h, st);
    else if (a.d <= 32) abh_launch_partial<AlsCfg<32, 1>, W>(a, h, st);
    else if (a.d <= 64) abh_launch_partial<AlsCfg<64, 4>, W>(a, h, st);
    else if (a.d <= 128) abh_launch_partial<AlsCfg<128, 4>, W>(a, h, st);
    else abh_launch_partial<AlsCfg<256, 4>, W>(a, h, st);
    MI_HIP(hipGetLastError());
    hipLaunchKernelGGL((abh_assemble_kernel<W>), dim3((unsigned)h.cap_rows, (unsigned)abh_tiles_of(a.d) + 1), dim3(256), 0, st, a, h);
    MI_HIP(hipGetLastError());
    const dim3 grid((unsigned)h.cap_rows), blk(MI_WAVE);
    if (block == 16) hipLaunchKernelGGL((abh_solve_kernel<16, W>), grid, blk, 0, st, a, h);
    else if (block == 32) hipLaunchKernelGGL((abh_solve_kernel<32, W>), grid, blk, 0, st, a, h);
    else hipLaunchKernelGGL((abh_solve_kernel<64, W>), grid, blk, 0, st, a, h);
    MI_HIP(hipGetLastError());
    return 0;
}

// The body of all four entries: W = false is the unweighted one (alpha, reg), W = true takes (conf, reg_rows or reg);
// with_hub = false is the entries without hub rows (the threshold and the hub counts are then not looked at).
template <bool W>
int ab_run(int64_t n_rows, int64_t d, int64_t block, int64_t sweeps, const int32_t* ptr, const int32_t* idx, int64_t nnz,
           int64_t n_cols, const float* Y, int64_t ldy, const float* G, float alpha, const float* conf, const float* reg_rows,
           float reg, float* X, int64_t ldx, int32_t from_zero, const int32_t* row_list, int64_t n_list, int32_t* n_failed,
           void* ws, size_t ws_bytes, mi_stream_t stream, bool with_hub = false, int64_t hub_threshold = 0,
           int64_t hub_rows = 0, int64_t hub_chunks = 0) {
    const int64_t lim = (int64_t)1 << 31;
    MI_CHECK_ARG(ab_shape_ok(d, block));
    MI_CHECK_ARG(!with_hub || abh_counts_ok(hub_threshold, hub_rows, hub_chunks));
    MI_CHECK_ARG(sweeps >= 1 && sweeps <= 64);
    MI_CHECK_ARG(n_rows >= 0 && n_rows < lim && n_cols >= 0 && n_cols < lim && nnz >= 0 && nnz < lim);
    if (W) {
        MI_CHECK_ARG(conf != nullptr);
        MI_CHECK_ARG(reg_rows != nullptr || (reg > 0.f && reg < INFINITY));
    } else {
        MI_CHECK_ARG(alpha >= 0.f && alpha < INFINITY && reg > 0.f && reg < INFINITY);
    }
    const int64_t n_work = row_list ? n_list : n_rows;
    MI_CHECK_ARG(n_work >= 0 && n_work < lim);
    MI_CHECK_ARG(n_failed != nullptr);
    if (n_work == 0) return 0;
    MI_CHECK_ARG(ptr && (idx || nnz == 0) && Y && G && X);
    MI_CHECK_ARG(mi_aligned16(Y) && ldy >= d && ldy % 4 == 0 && ldx >= d);
    const AbHubLayout lay = abh_layout(n_work, nnz, d, hub_rows, hub_chunks);
    if (!ws || ws_bytes < (with_hub ? lay.total : ab_ws_bytes(nnz, d))) return MI_ERR_WORKSPACE;
    AbArgs a;
    a.n_rows = (int)n_rows; a.d = (int)d; a.n_cols = (int)n_cols; a.n_work = (int)n_work; a.nnz = (int)nnz;
    a.sweeps = (int)sweeps; a.from_zero = from_zero != 0;
    a.ptr = ptr; a.idx = idx; a.Y = Y; a.ldy = ldy; a.alpha = alpha; a.reg = reg; a.X = X; a.ldx = ldx;
    a.row_list = row_list; a.n_failed = n_failed;
    a.conf = conf; a.reg_rows = reg_rows;
    a.Gs = static_cast<float*>(ws);
    a.pw = reinterpret_cast<float*>(static_cast<char*>(ws) + ab_ws_g(d));
    hipStream_t st = static_cast<hipStream_t>(stream);
    a.hub_thr = AB_NO_HUB;
    a.hub_slot = nullptr;
    hipLaunchKernelGGL(als_block_sym_kernel, dim3((unsigned)mi_ceil_div(d * d, 256)), dim3(256), 0, st, G, a.Gs, (int)d);
    MI_HIP(hipGetLastError());
    if (with_hub) {
        char* w = static_cast<char*>(ws);
        AbHub h;
        h.L = abh_chunk_of((int)d); h.cap_rows = (int)hub_rows; h.cap_chunks = (int)hub_chunks;
        h.counters = reinterpret_cast<int32_t*>(w + lay.counters);
        h.slot_of = reinterpret_cast<int32_t*>(w + lay.slot_of);
        h.row_pos = reinterpret_cast<int32_t*>(w + lay.row_pos);
        h.row_base = reinterpret_cast<int32_t*>(w + lay.row_base);
        h.chunk_row = reinterpret_cast<int32_t*>(w + lay.chunk_row);
        h.part = reinterpret_cast<float*>(w + lay.part);
        h.sys = reinterpret_cast<float*>(w + lay.sys);
        a.hub_thr = (int)hub_threshold;
        a.hub_slot = h.slot_of;
        const int rc = abh_run<W>(a, h, block, st);
        if (rc != 0) return rc;
    }
    const dim3 grid((unsigned)mi_ceil_div(n_work, AB_WAVES)), blk(AB_WAVES * MI_WAVE);
    if (block == 16) hipLaunchKernelGGL((als_block_kernel<16, W>), grid, blk, 0, st, a);
    else if (block == 32) hipLaunchKernelGGL((als_block_kernel<32, W>), grid, blk, 0, st, a);
    else hipLaunchKernelGGL((als_block_kernel<64, W>), grid, blk, 0, st, a);
    return mi_launch_status();
}

}  // namespace

extern "C" {

int32_t mi_als_block_chunk(int64_t d, int64_t block) { return ab_shape_ok(d, block) ? ab_res_of((int)d) : 0; }

size_t mi_als_block_rows_workspace_bytes(int64_t n_work, int64_t nnz, int64_t d, int64_t block) {
    if (n_work < 0 || nnz < 0 || nnz >= ((int64_t)1 << 31) || !ab_shape_ok(d, block)) return 0;
    return ab_ws_bytes(nnz, d);
}

int mi_als_block_rows_f32(int64_t n_rows, int64_t d, int64_t block, int64_t sweeps, const int32_t* ptr, const int32_t* idx,
                          int64_t nnz, int64_t n_cols, const float* Y, int64_t ldy, const float* G, float alpha, float reg,
                          float* X, int64_t ldx, int32_t from_zero, const int32_t* row_list, int64_t n_list, int32_t* n_failed,
                          void* ws, size_t ws_bytes, mi_stream_t stream) {
    return ab_run<false>(n_rows, d, block, sweeps, ptr, idx, nnz, n_cols, Y, ldy, G, alpha, nullptr, nullptr, reg, X, ldx,
                         from_zero, row_list, n_list, n_failed, ws, ws_bytes, stream);
}

size_t mi_als_block_rows_w_workspace_bytes(int64_t n_work, int64_t nnz, int64_t d, int64_t block) {
    return mi_als_block_rows_workspace_bytes(n_work, nnz, d, block);
}

int mi_als_block_rows_w_f32(int64_t n_rows, int64_t d, int64_t block, int64_t sweeps, const int32_t* ptr, const int32_t* idx,
                            int64_t nnz, int64_t n_cols, const float* Y, int64_t ldy, const float* G, const float* conf,
                            const float* reg_rows, float reg, float* X, int64_t ldx, int32_t from_zero, const int32_t* row_list,
                            int64_t n_list, int32_t* n_failed, void* ws, size_t ws_bytes, mi_stream_t stream) {
    return ab_run<true>(n_rows, d, block, sweeps, ptr, idx, nnz, n_cols, Y, ldy, G, 0.f, conf, reg_rows, reg, X, ldx, from_zero,
                        row_list, n_list, n_failed, ws, ws_bytes, stream);
}

int32_t mi_als_block_hub_chunk(int64_t d) { return ab_shape_ok(d, 16) ? abh_chunk_of((int)d) : 0; }

size_t mi_als_block_rows_hub_workspace_bytes(int64_t n_work, int64_t nnz, int64_t d, int64_t block, int64_t n_hub_rows,
                                             int64_t n_hub_chunks) {
    if (n_work < 0 || n_work >= ((int64_t)1 << 31) || nnz < 0 || nnz >= ((int64_t)1 << 31) || !ab_shape_ok(d, block) ||
        !abh_counts_ok(1, n_hub_rows, n_hub_chunks))
        return 0;
    return abh_layout(n_work, nnz, d, n_hub_rows, n_hub_chunks).total;
}

int mi_als_block_rows_hub_f32(int64_t n_rows, int64_t d, int64_t block, int64_t sweeps, const int32_t* ptr, const int32_t* idx,
                              int64_t nnz, int64_t n_cols, const float* Y, int64_t ldy, const float* G, float alpha, float reg,
                              float* X, int64_t ldx, int32_t from_zero, const int32_t* row_list, int64_t n_list,
                              int64_t hub_threshold, int64_t n_hub_rows, int64_t n_hub_chunks, int32_t* n_failed, void* ws,
                              size_t ws_bytes, mi_stream_t stream) {
    return ab_run<false>(n_rows, d, block, sweeps, ptr, idx, nnz, n_cols, Y, ldy, G, alpha, nullptr, nullptr, reg, X, ldx,
                         from_zero, row_list, n_list, n_failed, ws, ws_bytes, stream, true, hub_threshold, n_hub_rows,
                         n_hub_chunks);
}

size_t mi_als_block_rows_hub_w_workspace_bytes(int64_t n_work, int64_t nnz, int64_t d, int64_t block, int64_t n_hub_rows,
                                               int64_t n_hub_chunks) {
    return mi_als_block_rows_hub_workspace_bytes(n_work, nnz, d, block, n_hub_rows, n_hub_chunks);
}

int mi_als_block_rows_hub_w_f32(int64_t n_rows, int64_t d, int64_t block, int64_t sweeps, const int32_t* ptr,
                                const int32_t* idx, int64_t nnz, int64_t n_cols, const float* Y, int64_t ldy, const float* G,
                                const float* conf, const float* reg_rows, float reg, float* X, int64_t ldx, int32_t from_zero,
                                const int32_t* row_list, int64_t n_list, int64_t hub_threshold, int64_t n_hub_rows,
                                int64_t n_hub_chunks, int32_t* n_failed, void* ws, size_t ws_bytes, mi_stream_t stream) {
    return ab_run<true>(n_rows, d, block, sweeps, ptr, idx, nnz, n_cols, Y, ldy, G, 0.f, conf, reg_rows, reg, X, ldx, from_zero,
                        row_list, n_list, n_failed, ws, ws_bytes, stream, true, hub_threshold, n_hub_rows, n_hub_chunks);
}

}  // extern "C"
