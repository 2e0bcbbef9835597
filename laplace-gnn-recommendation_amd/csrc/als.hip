// Implicit ALS row solves (include/laplace_hip.h "iALS", additive to ABI 14): for every row of a CSR over a factor table Y, the
// d x d system  A = G + alpha * sum_e y_e y_e^T + reg I,  b = (1 + alpha) * sum_e y_e  is formed and solved by an f32 Cholesky
// factorisation, all inside one workgroup.  The numerics (chunks of L entries, one fmaf chain per chunk, chunks added in
// ascending order) are the header's rule; this comment is about the layout.
//
// Width classes.  d is padded to DP in {16, 32, 64, 128}; a class has WAVES = 1, 1, 4, 4 wavefronts per workgroup and ONE row per
// workgroup (a 64-thread workgroup at d <= 32, so that a 16 x 16 system does not hold four wavefronts).  d = 48 or 96 run in
// the next class and pay its tiles (the tiles wholly beyond d are skipped, their LDS rows are not).
//
// Rank-n update.  The lower triangle of S is cut into 16 x 16 tiles (DP / 16 (DP / 16 + 1) / 2 of them: 1, 3, 10, 36), dealt
// round-robin to the wavefronts (1, 3, 3, 9 tiles each, four accumulator registers per tile).  Entries are gathered KT = 32 at a
// time with 16-byte loads (DP / 4 float4 per entry, 2 or 4 per thread), the next 32 in flight in registers under the MFMAs of
// the current ones, and staged in LDS as [entry][column] rows.  v_mfma_f32_16x16x4_f32 takes A[i = lane & 15][k = lane >> 4] and
// B[k = lane >> 4][j = lane & 15]: with the ENTRIES as k, both operands of tile (ti, tj) are one ds_read_b32 each from the staged
// rows (columns 16 ti + i and 16 tj + j of entry 4 step + k), and the instruction adds entries 4 step .. 4 step + 3 to the
// accumulator in that order, one rounding per product: the rule's chain.  Entries past the end of the row are staged as zeros
// (fmaf(0, 0, acc) == acc).  s is summed by thread j < d from the same staged rows, in entry order.
// The staged rows have a stride of DP + 16 floats (16 at DP = 16), i.e. 16 mod 32 banks: the two entries x 16 columns that one
// half-wave of a ds_read_b32 touches fall on 32 different banks.
//
// Long rows (more than L entries).  A plan kernel gives every chunk of every long row a slot of the workspace (an INTEGER atomic
// on a counter: which slot a chunk gets may differ from run to run, what is written into it does not), a partial kernel — the
// same gather / MFMA code, one workgroup per chunk — writes (S_c, s_c) there, and the solving workgroup of the row adds them in
// ascending c into the registers the direct path leaves its single chunk in.  From there on both paths are one code.
//
// Factorisation.  A lives in LDS as [d + 1][DP + 16] floats (74 KiB at d = 128, two workgroups per CU of the 160 KiB; it ALIASES
// the staging rows, which are dead by then), row d holding b: a right-looking Cholesky that carries b along as an extra row is
// the forward substitution too (row d of L is y = L^-1 b).  It is blocked by panels of 16 columns.  Inside a panel the threads
// are a 16 x (NT / 16) grid over (column, row) and a step updates the panel's remaining columns only, one element per thread
// and row; one barrier per column: step k reads the UNSCALED column k from a small double-buffered copy (cb), scales on the fly
// by 1 / sqrt(pivot), and the threads that finish column k + 1 drop it into the other copy; L[i][k] itself is written where
// nobody reads it any more.  Behind a panel the trailing matrix takes A22 -= L21 L21^T by 16 x 16 tiles on the same matrix
// instruction as the rank-n update (the panel's 16 columns are k: four instructions per tile, the tile loaded from and stored
// to LDS in the C layout), b's entries beyond the panel by one thread each.  An element-wise trailing update was measured first:
// it is bound by the VALU instructions of its index arithmetic, not by LDS or the barriers (profiles/als.md).  The operand
// reads of the trailing tiles walk DOWN a column of L (stride DP + 16 floats: 8-way bank conflicts); they are 8 per tile.
// The backward substitution runs on wavefront 0 alone, x in two registers per lane, x_k handed round by a lane shuffle: no
// barrier.
// A pivot that is not a positive finite number is seen by every thread at once (all read the same word): the workgroup writes a
// zero row, thread 0 counts it, everybody leaves.  Nothing of that touches memory outside the row's own x.
//
// Weighted entry ("iALS weighted" in the header: a confidence a_e per entry, a regulariser per row).  The same kernels with
// W = true: als_accumulate_w stages a second image z = a y beside y (the B operand of every tile; same stride, same banks) and
// c_e = 1 + a_e for the s chain; A = (G + S) + reg_r I, b = s.  The system still aliases both images (64 staged rows <= d + 1
// rows at d >= 64; at d <= 32 the staging is the larger and the kernel's LDS doubles).  The W = false instantiations compile
// to the instructions they had before the parameter existed.  Measured: profiles/als_weighted.md.
//
// Measured rates and where this is poor (a user half-sweep is all factorisation: one barrier per column with four wavefronts
// waiting on it; the d <= 32 classes run one row per workgroup): profiles/als.md.
#include "common.hpp"
#include "als_gram.hpp"

namespace {

__host__ __device__ constexpr int als_chunk_of(int d) { return d <= 64 ? 4096 : 2048; }

struct AlsArgs {
    int n_rows, d, n_cols, n_work, nnz;
    const int32_t* ptr;
    const int32_t* idx;
    const float* Y;
    int64_t ldy;
    const float* G;
    float alpha, reg;
    float* X;
    int64_t ldx;
    const int32_t* row_list;
    int32_t* n_failed;
    int32_t* counter;      // workspace: chunk slots handed out
    int32_t* chunk_row;    // [cap]  slot -> work position, -1 = unused
    int32_t* chunk_base;   // [n_work]  first slot of a long row, -1 = none left
    float* part;           // [cap][d * d + d]
    int cap;
    const float* conf;     // weighted entries only: a_e by entry position
    const float* reg_rows; // weighted entries only: reg by ROW ID, or null (the scalar reg)
};

__global__ void als_plan_kernel(AlsArgs a, int L) {
    const int pos = blockIdx.x * blockDim.x + threadIdx.x;
    if (pos >= a.n_work) return;
    const int r = a.row_list ? a.row_list[pos] : pos;
    int base = -1;
    if ((unsigned)r < (unsigned)a.n_rows) {
        const int q0 = a.ptr[r], n = a.ptr[r + 1] - q0;
        if (n > L && q0 >= 0 && n <= a.nnz - q0) {
            const int nch = (n + L - 1) / L;
            const int b = atomicAdd(a.counter, nch);
            if (b >= 0 && b <= a.cap - nch) {
                base = b;
                for (int c = 0; c < nch; ++c) a.chunk_row[b + c] = pos;
            }
        }
    }
    a.chunk_base[pos] = base;
}

template <class C, bool W>
__global__ __launch_bounds__(C::NT) void als_partial_kernel(AlsArgs a) {
    __shared__ __align__(16) float sm[(W ? 2 : 1) * ALS_KT * C::LDA];
    const int slot = blockIdx.x;
    const int pos = a.chunk_row[slot];
    if (pos < 0) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int d = a.d, L = als_chunk_of(d);
    const int r = a.row_list ? a.row_list[pos] : pos;
    const int c = slot - a.chunk_base[pos];
    const int p0 = a.ptr[r] + c * L, p1 = min(p0 + L, a.ptr[r + 1]);
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
    float* out = a.part + (int64_t)slot * (d * d + d);
#pragma unroll
    for (int s = 0; s < C::TPW; ++s) {
        if (!live[s]) continue;
        const int col = 16 * tj[s] + (lane & 15);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int row = 16 * ti[s] + 4 * (lane >> 4) + g;
            if (row < d && col < d) out[row * d + col] = acc[s][g];
        }
    }
    if (tid < d) out[d * d + tid] = s_sum;
}

template <class C, bool W>
__global__ __launch_bounds__(C::NT) void als_solve_kernel(AlsArgs a) {
    __shared__ __align__(16) float sm[(W ? C::SM_ROWS_W : C::SM_ROWS) * C::LDA];   // the staged entries, then A with b as row d
    __shared__ float cb[2][C::DP + 1];                         // column k (unscaled) of the step that reads it
    __shared__ float dinv[C::DP];                              // 1 / L[k][k]
    const int tid = threadIdx.x, lane = tid & 63;
    const int d = a.d, L = als_chunk_of(d);
    const int pos = blockIdx.x;
    const int r = a.row_list ? a.row_list[pos] : pos;
    float* x = a.X + (int64_t)pos * a.ldx;
    int p0 = 0, n = 0;
    if ((unsigned)r < (unsigned)a.n_rows) {
        p0 = a.ptr[r];
        n = a.ptr[r + 1] - p0;
    }
    if (n <= 0) {
        if (tid < d) x[tid] = 0.f;
        return;
    }
    bool failed = p0 < 0 || n > a.nnz - p0;   // a rowptr that disagrees with nnz: nothing of idx is read for this row
    float reg_r = a.reg;
    if constexpr (W) {
        if (a.reg_rows) reg_r = a.reg_rows[r];   // by row id; r is inside [0, n_rows) here
        failed = failed || !(reg_r > 0.f && reg_r < INFINITY);
    }
    int ti[C::TPW], tj[C::TPW];
    bool live[C::TPW];
    f32x4 acc[C::TPW];
    als_tiles<C>(d, ti, tj, live);
#pragma unroll
    for (int s = 0; s < C::TPW; ++s) acc[s] = f32x4{0.f, 0.f, 0.f, 0.f};
    float s_sum = 0.f;
    if (failed) {
    } else if (n <= L) {
        if constexpr (W) {
            __shared__ float cs[ALS_KT];
            als_accumulate_w<C>(a, p0, p0 + n, sm, cs, ti, tj, live, acc, s_sum);
        } else {
            als_accumulate<C>(a, p0, p0 + n, sm, ti, tj, live, acc, s_sum);
        }
    } else {
        const int base = a.cap > 0 ? a.chunk_base[pos] : -1;   // -1: no slots left (a row listed twice); counted as failed
        failed = base < 0;
        const int nch = failed ? 0 : (n + L - 1) / L;
        for (int c = 0; c < nch; ++c) {
            const float* part = a.part + (int64_t)(base + c) * (d * d + d);
#pragma unroll
            for (int s = 0; s < C::TPW; ++s) {
                if (!live[s]) continue;
                const int col = 16 * tj[s] + (lane & 15);
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int row = 16 * ti[s] + 4 * (lane >> 4) + g;
                    if (row < d && col < d) acc[s][g] = acc[s][g] + part[row * d + col];
                }
            }
            if (tid < d) s_sum = s_sum + part[d * d + tid];
        }
    }
    // A = fmaf(alpha, S, G) + reg I (lower triangle), b = (1 + alpha) s as row d; weighted: A = (G + S) + reg_r I, b = s
    if (!failed) {
#pragma unroll
        for (int s = 0; s < C::TPW; ++s) {
            if (!live[s]) continue;
            const int col = 16 * tj[s] + (lane & 15);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int row = 16 * ti[s] + 4 * (lane >> 4) + g;
                if (row < d && col <= row) {
                    float v;
                    if constexpr (W) v = a.G[row * d + col] + acc[s][g];
                    else v = fmaf(a.alpha, acc[s][g], a.G[row * d + col]);
                    if (row == col) v = v + reg_r;
                    sm[row * C::LDA + col] = v;
                    if (col == 0) cb[0][row] = v;
                }
            }
        }
        if (tid < d) {
            const float bj = W ? s_sum : (1.0f + a.alpha) * s_sum;
            sm[d * C::LDA + tid] = bj;
            if (tid == 0) cb[0][d] = bj;
        }
    }
    __syncthreads();
    constexpr int TY = C::NT / 16;
    const int tx = tid & 15, ty = tid >> 4, wave = tid >> 6;
    for (int p0 = 0; p0 < d && !failed; p0 += 16) {
        const int pe = min(p0 + 16, d);   // the panel: columns [p0, pe)
        for (int k = p0; k < pe; ++k) {
            const float* c = cb[k & 1];
            float* nb = cb[(k + 1) & 1];
            const float p = c[k];
            if (!(p > 0.f && p < INFINITY)) {
                failed = true;   // every thread reads the same word: the whole workgroup leaves the loops here
                break;
            }
            const float inv = 1.0f / sqrtf(p);
            const int j = k + 1 + tx;   // the panel is 16 wide: one column per tx
            for (int i = k + 1 + ty; i <= d; i += TY) {
                const float li = c[i] * inv;
                if (tx == 0) sm[i * C::LDA + k] = li;
                if (j <= min(i, pe - 1)) {
                    const float v = fmaf(-li, c[j] * inv, sm[i * C::LDA + j]);
                    sm[i * C::LDA + j] = v;
                    if (tx == 0) nb[i] = v;
                }
            }
            if (tid == 0) dinv[k] = inv;
            __syncthreads();
        }
        if (failed || pe >= d) break;
        // trailing update A22 -= L21 L21^T by 16 x 16 tiles on the matrix instruction, the panel's 16 columns as k; pe is a
        // multiple of 16 here.  Row d (b) is not a tile row: its entries beyond the panel are updated by one thread each.
        {
            const int T0 = pe >> 4, TN = ((d + 15) >> 4) - T0, ntile = TN * (TN + 1) / 2;
            const int arow = lane & 15, ak = lane >> 4;
            for (int q = wave; q < ntile; q += C::WAVES) {
                int ti, tj;
                als_tile_of(q, ti, tj);
                ti += T0;
                tj += T0;
                const int col = 16 * tj + (lane & 15), row0 = 16 * ti + 4 * (lane >> 4);
                f32x4 t4;
#pragma unroll
                for (int g = 0; g < 4; ++g) t4[g] = sm[(row0 + g) * C::LDA + col];
                const float* pa = sm + (16 * ti + arow) * C::LDA + p0 + ak;
                const float* pb = sm + (16 * tj + arow) * C::LDA + p0 + ak;
#pragma unroll
                for (int s4 = 0; s4 < 4; ++s4) t4 = __builtin_amdgcn_mfma_f32_16x16x4f32(-pa[4 * s4], pb[4 * s4], t4, 0, 0, 0);
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    if (row0 + g < d && col <= row0 + g) sm[(row0 + g) * C::LDA + col] = t4[g];
                }
            }
            for (int jb = pe + tid; jb < d; jb += C::NT) {
                float v = sm[d * C::LDA + jb];
                for (int k = p0; k < pe; ++k) v = fmaf(-sm[d * C::LDA + k], sm[jb * C::LDA + k], v);
                sm[d * C::LDA + jb] = v;
            }
        }
        __syncthreads();
        for (int i = pe + tid; i <= d; i += C::NT) cb[pe & 1][i] = sm[i * C::LDA + pe];   // column pe, unscaled, for step pe
        __syncthreads();
    }
    if (failed) {
        if (tid < d) x[tid] = 0.f;
        if (tid == 0) atomicAdd(a.n_failed, 1);
        return;
    }
    if (tid < 64) {   // L^T x = y on wavefront 0; lane l keeps elements l and l + 64
        float y0 = lane < d ? sm[d * C::LDA + lane] : 0.f;
        float y1 = lane + 64 < d ? sm[d * C::LDA + lane + 64] : 0.f;
        for (int k = d - 1; k >= 0; --k) {
            const float xk = __shfl(k < 64 ? y0 : y1, k & 63, MI_WAVE) * dinv[k];
            if (lane == (k & 63)) {
                if (k < 64) y0 = xk; else y1 = xk;
            }
            const float* lk = sm + k * C::LDA;
            if (lane < k) y0 = fmaf(-lk[lane], xk, y0);
            if (lane + 64 < k) y1 = fmaf(-lk[lane + 64], xk, y1);
        }
        if (lane < d) x[lane] = y0;
        if (lane + 64 < d) x[lane + 64] = y1;
    }
}

inline int64_t als_cap(int64_t nnz, int L) { return nnz / L + nnz / (L + 1); }   // >= sum of ceil(n / L) over rows with n > L

struct AlsLayout {
    size_t counter, chunk_row, chunk_base, part, total;
};
inline AlsLayout als_layout(int64_t n_work, int64_t nnz, int64_t d) {
    const int64_t cap = als_cap(nnz, als_chunk_of((int)d));
    AlsLayout l;
    l.counter = 0;
    l.chunk_row = 256;
    l.chunk_base = l.chunk_row + mi_align_up((size_t)cap * 4, 256);
    l.part = l.chunk_base + mi_align_up((size_t)n_work * 4, 256);
    l.total = l.part + mi_align_up((size_t)cap * (size_t)(d * d + d) * 4, 256);
    return l;
}

inline bool als_width_ok(int64_t d) { return d >= 4 && d <= 128 && d % 4 == 0; }

template <class C, bool W>
int als_launch(const AlsArgs& a, hipStream_t st) {
    if (a.cap > 0) {
        hipLaunchKernelGGL((als_partial_kernel<C, W>), dim3(a.cap), dim3(C::NT), 0, st, a);
        MI_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL((als_solve_kernel<C, W>), dim3(a.n_work), dim3(C::NT), 0, st, a);
    return mi_launch_status();
}

// The body of both entries: conf == null is the unweighted one (alpha, reg), otherwise (conf, reg_rows or reg).
template <bool W>
int als_run(int64_t n_rows, int64_t d, const int32_t* ptr, const int32_t* idx, int64_t nnz, int64_t n_cols, const float* Y,
            int64_t ldy, const float* G, float alpha, const float* conf, const float* reg_rows, float reg, float* X, int64_t ldx,
            const int32_t* row_list, int64_t n_list, int32_t* n_failed, void* ws, size_t ws_bytes, mi_stream_t stream) {
    const int64_t lim = (int64_t)1 << 31;
    MI_CHECK_ARG(als_width_ok(d));
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
    const AlsLayout lay = als_layout(n_work, nnz, d);
    if (!ws || ws_bytes < lay.total) return MI_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    char* w = static_cast<char*>(ws);
    AlsArgs a;
    a.n_rows = (int)n_rows; a.d = (int)d; a.n_cols = (int)n_cols; a.n_work = (int)n_work; a.nnz = (int)nnz;
    a.ptr = ptr; a.idx = idx; a.Y = Y; a.ldy = ldy; a.G = G; a.alpha = alpha; a.reg = reg; a.X = X; a.ldx = ldx;
    a.row_list = row_list; a.n_failed = n_failed;
    a.conf = conf; a.reg_rows = reg_rows;
    a.counter = reinterpret_cast<int32_t*>(w + lay.counter);
    a.chunk_row = reinterpret_cast<int32_t*>(w + lay.chunk_row);
    a.chunk_base = reinterpret_cast<int32_t*>(w + lay.chunk_base);
    a.part = reinterpret_cast<float*>(w + lay.part);
    a.cap = (int)als_cap(nnz, als_chunk_of((int)d));
    if (a.cap > 0) {
        MI_HIP(hipMemsetAsync(a.counter, 0, 256, st));
        MI_HIP(hipMemsetAsync(a.chunk_row, 0xFF, (size_t)a.cap * 4, st));
        hipLaunchKernelGGL(als_plan_kernel, dim3((unsigned)mi_ceil_div(n_work, 256)), dim3(256), 0, st, a, als_chunk_of((int)d));
        MI_HIP(hipGetLastError());
    }
    if (d <= 16) return als_launch<AlsCfg<16, 1>, W>(a, st);
    if (d <= 32) return als_launch<AlsCfg<32, 1>, W>(a, st);
    if (d <= 64) return als_launch<AlsCfg<64, 4>, W>(a, st);
    return als_launch<AlsCfg<128, 4>, W>(a, st);
}

}  // namespace

extern "C" {

int32_t mi_als_chunk(int64_t d) { return als_width_ok(d) ? als_chunk_of((int)d) : 0; }

size_t mi_als_solve_rows_workspace_bytes(int64_t n_work, int64_t nnz, int64_t d) {
    if (n_work < 0 || nnz < 0 || nnz >= ((int64_t)1 << 31) || !als_width_ok(d)) return 0;
    return als_layout(n_work, nnz, d).total;
}

int mi_als_solve_rows_f32(int64_t n_rows, int64_t d, const int32_t* ptr, const int32_t* idx, int64_t nnz, int64_t n_cols,
                          const float* Y, int64_t ldy, const float* G, float alpha, float reg, float* X, int64_t ldx,
                          const int32_t* row_list, int64_t n_list, int32_t* n_failed, void* ws, size_t ws_bytes,
                          mi_stream_t stream) {
    return als_run<false>(n_rows, d, ptr, idx, nnz, n_cols, Y, ldy, G, alpha, nullptr, nullptr, reg, X, ldx, row_list, n_list,
                          n_failed, ws, ws_bytes, stream);
}

size_t mi_als_solve_rows_w_workspace_bytes(int64_t n_work, int64_t nnz, int64_t d) {
    return mi_als_solve_rows_workspace_bytes(n_work, nnz, d);
}

int mi_als_solve_rows_w_f32(int64_t n_rows, int64_t d, const int32_t* ptr, const int32_t* idx, int64_t nnz, int64_t n_cols,
                            const float* Y, int64_t ldy, const float* G, const float* conf, const float* reg_rows, float reg,
                            float* X, int64_t ldx, const int32_t* row_list, int64_t n_list, int32_t* n_failed, void* ws,
                            size_t ws_bytes, mi_stream_t stream) {
    return als_run<true>(n_rows, d, ptr, idx, nnz, n_cols, Y, ldy, G, 0.f, conf, reg_rows, reg, X, ldx, row_list, n_list,
                         n_failed, ws, ws_bytes, stream);
}

}  // extern "C"
