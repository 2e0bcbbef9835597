/*
 * laplace_hip.h — C ABI of liblaplace_hip.so, the MI355X (gfx950) hot path of the
 * laplace GNN link-prediction engine.
 *
 * The reference (dream-faster/laplace-gnn-recommendation) has no FFI of its own: its
 * hot path reaches native code only through third-party wheels (torch_sparse,
 * torch_scatter, PyG).  Each entry point below replaces one of those call sites; the
 * "replaces:" line cites the reference file:line (paths relative to the reference root)
 * whose work it does.  INTEGRATION.md shows the ctypes binding a reference maintainer
 * would add at each site.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer owned by the caller unless marked "host";
 *  - every function enqueues on `stream` (a hipStream_t passed as void*) and returns
 *    without synchronising, except the *_plan_build / *_count functions, which say so;
 *  - return value: 0 = success; >0 = hipError_t from the runtime; <0 = MI_ERR_* below;
 *  - no global mutable state: the library is re-entrant and thread-safe;
 *  - node / edge indices inside the library are int32 (n, nnz < 2^31 is checked);
 *    edge lists coming from the reference's tensors are int64 and converted once
 *    in mi_coo_to_csr_i32;
 *  - floating point is fp32 end to end (the reference's dtype); no reduced precision.  (Opt-in exceptions, each with a
 *    stated rule: top-K's bf16 prefilter, and the bf16 layer tables of the LightGCN forward at the end of this file.)
 */
#ifndef LAPLACE_HIP_H
#define LAPLACE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI_ABI_VERSION 14

#define MI_ERR_BAD_ARG      (-1)  /* null pointer, negative size, misaligned buffer   */
#define MI_ERR_TOO_LARGE    (-2)  /* a size does not fit int32 indexing                */
#define MI_ERR_WORKSPACE    (-3)  /* workspace smaller than *_workspace_bytes says     */
#define MI_ERR_UNSUPPORTED  (-4)  /* feature width / k outside the compiled kernels    */

typedef void* mi_stream_t; /* hipStream_t */

int         mi_abi_version(void);
const char* mi_error_string(int code); /* host string, static storage */

/* ------------------------------------------------------------------------------------
 * K4  COO -> sorted CSR.
 * replaces: torch_sparse.SparseTensor(row=, col=, sparse_sizes=) at
 *           data/lightgcn_loader.py:65-79 (sort by row*N+col, no duplicate merging,
 *           rowptr = ind2ptr(row)).
 * row/col: int64[nnz] as the reference's edge_index rows.  Outputs: rowptr int32[n_rows+1],
 * col_out int32[nnz] (sorted by (row, col)), perm int32[nnz] (perm[p] = index of the
 * input edge now at position p; nullable).
 * ---------------------------------------------------------------------------------- */
size_t mi_coo_to_csr_workspace_bytes(int64_t n_rows, int64_t nnz);
int    mi_coo_to_csr_i32(int64_t n_rows, int64_t n_cols, int64_t nnz,
                         const int64_t* row, const int64_t* col,
                         int32_t* rowptr, int32_t* col_out, int32_t* perm,
                         void* ws, size_t ws_bytes, mi_stream_t stream);

/* CSR(A) -> CSR(A^T).  replaces: SparseTensor.csr2csc()/colptr used by the backward of
 * torch_sparse.matmul (autograd through model/lightgcn.py:64).  perm_t[q] = position in
 * A of the entry now at position q of A^T (so val_t = val[perm_t]). */
size_t mi_csr_transpose_workspace_bytes(int64_t n_rows, int64_t nnz);
int    mi_csr_transpose_i32(int64_t n_rows, int64_t n_cols, int64_t nnz,
                            const int32_t* rowptr, const int32_t* col,
                            int32_t* rowptr_t, int32_t* col_t, int32_t* perm_t,
                            void* ws, size_t ws_bytes, mi_stream_t stream);

/* out[i] = src[idx[i]] — used to permute edge values. */
int mi_gather_f32(int64_t n, const float* src, const int32_t* idx, float* out,
                  mi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * K3  gcn_norm on a square CSR.
 * replaces: torch_geometric gcn_norm(SparseTensor, add_self_loops=False) at
 *           model/lightgcn.py:56:  deg = rowsum(A); dis = deg^-1/2 (inf -> 0);
 *           val[p] = (val[p] * dis[row]) * dis[col[p]].
 * val_in nullable (= all ones, SparseTensor without value).  dis_out float[n] is written
 * (deg^-1/2) and may be reused by the caller.
 * ---------------------------------------------------------------------------------- */
int mi_gcn_norm_csr_f32(int64_t n, int64_t nnz, const int32_t* rowptr, const int32_t* col,
                        const float* val_in, float* val_out, float* dis_out,
                        mi_stream_t stream);

/* Edge re-weighting: val_out[p] = (val_in[p] * row_scale[row(p)]) * col_scale[col[p]], any null
 * input meaning all ones.  gcn_norm is this with row_scale = col_scale = deg^-1/2; the
 * user-sharded multi-GPU path calls it directly because an item's degree is the sum over all
 * shards (one RCCL all-reduce of the degree vector at set-up), and SAGEConv's mean aggregation
 * (model/layers.py:11-24, aggr="mean") is row_scale = 1/in-degree. */
int mi_scale_csr_f32(int64_t n_rows, int64_t nnz, const int32_t* rowptr, const int32_t* col,
                     const float* val_in, const float* row_scale, const float* col_scale,
                     float* val_out, mi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * K1/K2  CSR SpMM with fused epilogue — the LightGCN propagate.
 * replaces: torch_sparse.matmul(adj_t, x) at model/lightgcn.py:87 (called K times per
 *           forward at :63-65, and K times on A^T in backward), plus the
 *           stack/mean at model/lightgcn.py:67-68 through the epilogue.
 *
 *   acc[r,:] = sum_{p in [rowptr[r], rowptr[r+1])} val[p] * X[col[p], :]
 *   if (Y) Y[r,:] = acc
 *   if (S) S[r,:] = scale * ((addend ? addend[r,:] : 0) + acc)
 *
 * d (feature width) must be a multiple of 4 and <= 512; X, Y, addend, S rows are
 * 16-byte aligned with leading dimensions ld* (in floats, multiples of 4).  S may alias
 * addend (in-place running sum).  Y/S must not alias X.
 *
 * Rows longer than the plan's chunk are split into work items whose partial sums are
 * reduced in a fixed order (no float atomics): results are bitwise reproducible run to run.
 * A BANDED plan (band > 0; needs `col`, columns ascending within each row) also cuts the
 * split rows at multiples of `band` columns and launches the work items band by band, the
 * workgroups of one band on one XCD, so that the gathers the hub rows make into the same
 * band of X meet in that XCD's L2 (choose band * d * 4 bytes ~ the 4 MB L2).  The plan
 * depends only on the adjacency structure; build it once.
 * ---------------------------------------------------------------------------------- */
#define MI_SPMM_GROUP 32   /* launch slots per XCD-interleave block of a banded plan */

typedef struct mi_spmm_plan {
    int32_t  chunk;        /* max nnz per work item of a split row                   */
    int32_t  n_long_rows;  /* rows with more than `chunk` entries                    */
    int32_t  n_items;      /* work items over all long rows = partial-sum rows       */
    int32_t  n_launch;     /* launch slots >= n_items (banded: a multiple of 8 * MI_SPMM_GROUP) */
    int32_t* long_rows;    /* device int32[n_long_rows]                              */
    int32_t* item_ptr;     /* device int32[n_long_rows+1]: slots of long row i       */
    int32_t* items;        /* device int32[4*n_launch], 16-byte aligned, in LAUNCH order:
                              row, begin, end, slot; slot < 0 = padding              */
    int32_t* long_index;   /* device int32[n_rows]: index into long_rows, -1 for
                              short rows; nullable (needed only by row_list launches)  */
    int32_t  band;         /* columns per band; 0 = row-major launch order           */
    int32_t  n_bands;
    /* Optional (round 4; all three or none): the split rows' entries copied into LAUNCH order by
     * mi_spmm_plan_pack_entries.  A work item's ~12 entries are then read from the same cache lines as its launch
     * neighbours' instead of two lines of their own in the CSR arrays (7.7 M work items on BASELINE configs[3]: ~2 GB of
     * line fetches per launch for 0.7 GB of entries).  epos[q] = first packed entry of launch slot q.  ecol / eval hold
     * VALUES: when the CSR's val changes, call mi_spmm_plan_pack_entries again with values_only = 1.                    */
    int32_t* epos;         /* device int32[n_launch]; nullable                       */
    int32_t* ecol;         /* device int32[nnz_long]                                 */
    float*   eval;         /* device float[nnz_long]                                 */
} mi_spmm_plan;

/* What mi_spmm_plan_count found; the caller allocates the plan arrays from it. */
typedef struct mi_spmm_plan_info {
    int64_t n_long_rows, n_items, n_launch, nnz_long;
    int32_t chunk, band, n_bands, queue_len;
    int32_t queue_start[9];
    int32_t keys_in_second;
} mi_spmm_plan_info;

/* Two phases, both SYNCHRONISE `stream` (counter read-backs); set-up time only.
 *   count: analyses the adjacency into `ws` and reports the array sizes in `info`;
 *   fill:  writes plan->long_rows[n_long_rows], item_ptr[n_long_rows+1], items[4*n_launch],
 *          long_index[n_rows] (nullable) — caller-allocated — and the scalar fields.
 * `ws` (mi_spmm_plan_workspace_bytes; worst case ~28 B per entry) must be the same buffer,
 * untouched in between.  col may be null when band == 0. */
size_t mi_spmm_plan_workspace_bytes(int64_t n_rows, int64_t nnz);
int    mi_spmm_plan_count(int64_t n_rows, int64_t n_cols, const int32_t* rowptr, const int32_t* col,
                          int32_t chunk, int32_t band, void* ws, size_t ws_bytes,
                          mi_spmm_plan_info* info, mi_stream_t stream);
/* The same analysis restricted to the rows with chunk < degree <= max_deg (round 4): the banded half of a HYBRID plan whose
 * rows above max_deg are laid out in SWEEP form (mi_spmm_sweep) by the host.  The host merges the two: long_rows / item_ptr
 * concatenated, the work items' slots shifted behind the sweep's 8 * n_slots partial rows, n_items = the sum; passing both
 * `items` and a sweep to mi_spmm_csr_ex_f32 runs both split-row kernels and ONE fix-up. */
int    mi_spmm_plan_count_range(int64_t n_rows, int64_t n_cols, const int32_t* rowptr, const int32_t* col,
                                int32_t chunk, int32_t max_deg, int32_t band, void* ws, size_t ws_bytes,
                                mi_spmm_plan_info* info, mi_stream_t stream);
/* The same analysis with a third row class: THIN rows, chunk < degree <= thin_max, get no work items and no partial rows —
 * only the rows with max(chunk, thin_max) < degree <= max_deg are split (thin_max = 0: mi_spmm_plan_count_range, bit for
 * bit).  A thin row holds a few entries per band, so as work items it pays a partial row for nearly every gather; it is
 * summed whole by a wavefront instead (mi_spmm_ex.thin_rows).  The caller lists the thin rows itself (degrees from rowptr),
 * longest first, marks them with -2 in plan->long_index after mi_spmm_plan_fill, and passes the list with EVERY launch of
 * the plan: neither the short-row nor the split-row kernels compute them. */
int    mi_spmm_plan_count_thin(int64_t n_rows, int64_t n_cols, const int32_t* rowptr, const int32_t* col,
                               int32_t chunk, int32_t thin_max, int32_t max_deg, int32_t band, void* ws, size_t ws_bytes,
                               mi_spmm_plan_info* info, mi_stream_t stream);
int    mi_spmm_plan_fill(int64_t n_rows, const int32_t* rowptr, const mi_spmm_plan_info* info,
                         mi_spmm_plan* plan, void* ws, size_t ws_bytes, mi_stream_t stream);
/* Fills plan->epos / ecol / eval (caller-allocated: n_launch, nnz_long, nnz_long elements; nnz_long from
 * mi_spmm_plan_info) from the filled plan and the CSR's col / val.  values_only != 0: epos and ecol are kept, eval is
 * copied again (the adjacency was re-weighted).  ws: mi_spmm_plan_pack_workspace_bytes(plan->n_launch).  Enqueues only. */
size_t mi_spmm_plan_pack_workspace_bytes(int64_t n_launch);
int    mi_spmm_plan_pack_entries(const mi_spmm_plan* plan, int64_t nnz_long, const int32_t* col, const float* val,
                                 int32_t values_only, void* ws, size_t ws_bytes, mi_stream_t stream);
/* Bytes of partial-sum workspace mi_spmm_csr_f32 needs for this plan and width. */
size_t mi_spmm_workspace_bytes(const mi_spmm_plan* plan, int64_t d);

int mi_spmm_csr_f32(int64_t n_rows, int64_t d,
                    const int32_t* rowptr, const int32_t* col, const float* val,
                    const float* X, int64_t ldx,
                    float* Y, int64_t ldy,
                    const float* addend, int64_t lda,
                    float* S, int64_t lds, float scale,
                    const mi_spmm_plan* plan, void* ws, size_t ws_bytes,
                    mi_stream_t stream);

/* Sparse-operand form of the same product — same arithmetic, fewer bytes.  Used by the fused
 * train step, where the operands around the K propagates are known to be mostly zero rows
 * (the BPR gradient touches <= 3*batch rows) or only a few output rows are consumed (the last
 * forward layer feeds only the batch rows of the loss).  Every field is nullable:
 *   x_map      int32[n_cols]: X is COMPACT; column c reads X[x_map[c]], and x_map[c] < 0
 *              declares row c of the logical X to be all zeros (its entries are skipped —
 *              adding exact zeros changes no sum).
 *   addend_map int32[n_rows]: addend is COMPACT; row r adds addend[addend_map[r]], < 0 = none.
 *   row_list   int32[n_list]: only these rows are computed; Y, S and addend are COMPACT,
 *              indexed by position in the list (addend_map must be null).  n_list is the launch
 *              bound; n_list_dev (device int32[1], nullable) the actual count, so that a
 *              device-built list needs no host read-back.  Needs plan->long_index when the plan
 *              has split rows.
 * Results equal the dense call on the corresponding dense operands bit for bit (up to the
 * sign of zero). */
/* Optimizer epilogue: the product's S value g[r,:] = scale * (addend[r,:] + acc) is the gradient of
 * parameter row r and is consumed in registers by the Adam update of mi_adam_dense_f32 (same arithmetic,
 * bit for bit) instead of being written and read back: p / m / v rows are updated in place, reg_w as
 * there.  S may be null (the gradient is then never stored).  p must not alias X, Y, S or addend. */
typedef struct mi_adam_args {
    float*       p;  int64_t ldp;   /* [n_rows, d] parameters, ld in floats */
    float*       m;                 /* [n_rows, d] dense */
    float*       v;                 /* [n_rows, d] dense */
    const float* reg_w;             /* [n_rows] or null */
    double       lr, beta1, beta2, eps;
    int64_t      step;              /* counts from 1 */
} mi_adam_args;

/* SWEEP form of the split-row half (round 2).  The banded work items above pay one partial row per (row, band)
 * pair, which forbids bands small enough to sit comfortably in an XCD's 4 MB L2, and their short (col, val) segments
 * are re-fetched by every XCD that holds a neighbouring band.  Here the entries of the long rows are re-laid out ONCE
 * into 8 * n_streams STREAMS — stream (x, k) = everything sub-group k of XCD x will ever process: the entries whose
 * column band is congruent to x mod 8, of the <= 8 row parts ("slots") that sub-group owns, sorted by band, then slot —
 * so each sub-group reads its (col, val) pairs as one contiguous run, walks the bands in step with its XCD's other
 * sub-groups (streams are balanced per band), keeps its <= 8 accumulators in LDS across ALL bands, and writes one
 * partial row per (slot, XCD) at the end: 8 * n_slots partial rows whatever the band size.  The plan's long_rows /
 * item_ptr / long_index / chunk keep their meaning (item_ptr[i] = 8 * first slot of long row i; n_items = 8 * n_slots)
 * and the same fix-up kernel reduces them in (slot, XCD) order: no float atomics, bitwise reproducible.
 * Feature widths up to 128 (one float4 per lane); wider products use the work-item form. */
typedef struct mi_spmm_sweep {
    const int32_t* col;         /* int32[nnz_long], stream order: bits 28..30 = accumulator of the owning sub-group (0..7),
                                   bit 27 = first entry of a new band in this stream, bits 0..26 = column                */
    const float*   val;         /* float[nnz_long], stream order                                                        */
    const int32_t* stream_ptr;  /* int32[8 * n_streams + 1]: stream (x, k) = entries [ptr[x*n_streams+k], ptr[..+1])    */
    const int32_t* slot_of;     /* int32[n_streams * 8]: slot held in accumulator q of sub-group k; < 0 = unused        */
    int32_t        n_streams;   /* sub-groups per XCD: a multiple of 32, at most 32 * 32                                */
    int32_t        n_slots;
    int32_t*       progress;    /* reserved (null)                                                                          */
    int32_t        epoch;       /* bands per XCD of the plan (read by the MI_SWEEP_WG_SYNC experiment build only; else ignored)      */
    int32_t        slack;       /* pacing: ticks of the 100 MHz device clock per band; wavefronts do not start band t before
                                   t * slack ticks after their start (a late wavefront never waits).  0 = no pacing.  For the
                                   L2 hit rate only: results do not depend on it                                          */
} mi_spmm_sweep;

/* TILES form of the hub rows (the longest split rows of an adjacency whose columns are far more than the L2s hold: the
 * item rows of a [users; items] graph).  A hub row has an entry in almost every tile of 64 or 128 consecutive rows of X, so
 * its gathers need no cache at all: P workgroups each own a contiguous run of whole tiles, stream every tile that holds a hub
 * entry through LDS ONCE, and add its entries into accumulators that stay in registers from the first tile to the last.
 * Layout, built once per adjacency (host: ops.build_hub_tiles_plan):
 *   slots      a slot is one accumulator: a hub row, or class j % k of the entries of a hub row (entry j of the row, k classes)
 *              where the row is heavier than the mean load of a sub-group — no slot is heavier than total hub entries / 32;
 *   sub-groups a workgroup is 32 sub-groups (one row of X wide: d / 4 lanes rounded up to 8, 16 or 32) of 16 accumulators;
 *              slots are assigned by longest-processing-time over their entry counts, slot_of[sg * 16 + a] (< 0 = unused);
 *   ranges     workgroup w owns the loaded tiles [wg_ptr[w], wg_ptr[w + 1]) of the list tile_id (tiles without a hub entry
 *              are not listed and never loaded); the cuts balance a modelled cost, not row counts;
 *   entries    tile j of the list owns entries [tile_ent[j], tile_ent[j + 1]) of ecol (column minus the tile's first) / eval,
 *              sorted by (sub-group, accumulator, column); cnt[(j * 32 + sg) * 16 + a] of them belong to accumulator a of
 *              sub-group sg, the sub-group's first is sg_off[j * 32 + sg] entries into the tile's run.
 * Reproducibility: everything is static.  Partial row (slot, w) = the slot's entries in w's range, added one by one in column
 * order; they sit at [slot * n_wg + w] IN FRONT of the work items' partial rows, plan->item_ptr / long_rows list the hub rows
 * first (item_ptr[i] = n_wg * first slot of hub row i), and the one fix-up kernel reduces them with every other split row in
 * its fixed order: no float atomics, nothing between workgroups, bitwise the same run to run and on one or two streams.
 * eval holds VALUES: re-copy it when the CSR's val changes.  Dense launches only (no x_map, no row_list), d <= 128. */
typedef struct mi_spmm_tiles {
    const uint8_t* ecol;        /* uint8[n_entries]                                                                      */
    const float*   eval;        /* float[n_entries]                                                                      */
    const int32_t* tile_id;     /* int32[n_listed]: tile number (first row of X = tile_id * tile), ascending              */
    const int32_t* tile_ent;    /* int32[n_listed + 1]                                                                   */
    const uint8_t* cnt;         /* uint8[n_listed * 32 * 16], 16-byte aligned                                            */
    const int32_t* sg_off;      /* int32[n_listed * 32]                                                                  */
    const int32_t* wg_ptr;      /* int32[n_wg + 1]                                                                       */
    const int32_t* slot_of;     /* int32[32 * 16]                                                                        */
    int32_t        n_wg;        /* P: workgroups = partial rows per slot                                                 */
    int32_t        n_slots;     /* 1 .. 512                                                                              */
    int32_t        tile;        /* 64 or 128                                                                             */
    int32_t        nt;          /* != 0: the streamed loads (X rows, entries) use the non-temporal policy                 */
    int64_t        n_cols;      /* rows of X                                                                             */
    int32_t        max_tile_entries;  /* largest tile_ent[j + 1] - tile_ent[j]; beyond 96 * sub-group lanes: MI_ERR_UNSUPPORTED */
} mi_spmm_tiles;

typedef struct mi_spmm_ex {
    const int32_t* x_map;
    const int32_t* addend_map;
    const int32_t* row_list;
    const int32_t* n_list_dev;
    int64_t        n_list;
    const mi_adam_args* adam;       /* nullable; not with row_list */
    int32_t        parts;           /* 0 = the whole product; else a mask: MI_SPMM_SHORT_ROWS computes the rows of at most
                                       plan->chunk entries, MI_SPMM_SPLIT_ROWS the split rows (work items + fix-up).  The two
                                       halves touch disjoint output rows, so a caller may enqueue them on two streams */
    int32_t        hot_rows;        /* 0 (the default, also of a null mi_spmm_ex and of mi_spmm_csr_f32): the plain
                                       one-workgroup-per-8-rows short-row launch — the measured best (profiles/
                                       r03_spmm_rows_persistent.md, r04_c4_item_rows_experiments.md).  != 0 (opt-in, dense launches
                                       with a plan, d <= 256): the short rows run as a PERSISTENT, software-pipelined launch — the
                                       grid is what the chip holds at once, wavefronts stride over the row pairs and fetch the next
                                       rows' pointers and (col, val) entries under the current gathers; hot_rows > 0 adds an LDS
                                       cache: rows [hot_base, hot_base + hot_rows) of X are staged once per workgroup and gathers
                                       of them are served from LDS instead of L2 (a recommendation graph under the locality order
                                       keeps its most popular items in the first item rows: 64 rows take ~46 %, 300 rows ~59 % of
                                       all user-row gathers), clipped to the workgroup's LDS share; hot_rows < 0 = persistent
                                       without a cache.  Hints for speed only: same values summed in the same order, bitwise the
                                       same result in all three forms.  (Round 3 had 0 = persistent and < 0 = plain: a zero-
                                       initialised struct silently chose the slower form.) */
    const mi_spmm_sweep* sweep;     /* nullable: the split rows run in SWEEP form (plan->items is then unused) */
    int32_t        hot_base;        /* first cached row of X (see hot_rows) */
    int32_t        hot_threads;     /* tuning of the hot-row launch, 0 = defaults: bits 0..11 workgroup size (256 / 512 / 1024),
                                       bits 12.. wavefronts per CU (workgroups per CU = that / wavefronts per workgroup) */
    const uint32_t* x_bits;         /* nullable, with x_map: bit c of the array (word c / 32, bit c % 32; mi_map_live_bits_i32 writes
                                       it) = (x_map[c] >= 0).  Saying so declares the live columns RARE (the batch's users among all
                                       users: first backward product of the fused step).  On a PACKED plan (epos / ecol / eval) the
                                       split rows' work items are then not walked one by one: wavefronts scan the packed entries,
                                       test the bit before the map, gather only the live entries in list order, write no partial
                                       row for a work item without any, and the fix-up skips those — same sums in the same order,
                                       bitwise the result without the hint.  Ignored with a sweep, a row_list or an unpacked plan. */
    const int32_t* thin_rows;       /* device int32[n_thin], with a plan from mi_spmm_plan_count_thin: its thin rows, longest first.
                                       Each is summed whole by one wavefront — equal consecutive pieces of the row, one per
                                       sub-group, added in sub-group order through LDS, one epilogue — as part of
                                       MI_SPMM_SPLIT_ROWS: no partial rows, no atomics, bitwise reproducible.  Serves every form
                                       (x_map, addend_map, adam; with row_list the listed rows whose long_index is -2) */
    int32_t        n_thin;          /* 0 (and a null mi_spmm_ex) = the plan has no thin rows */
    int32_t        row_slices;      /* 0 or 1 (and a null mi_spmm_ex) = the short-row launch as it is; 2 or 4 (anything else is
                                       MI_ERR_BAD_ARG) = its SLICED form for adjacencies whose short rows gather popularity-ordered
                                       rows (the user rows of a recommendation graph): the workgroup on XCD x (blockIdx.x & 7)
                                       computes column slice x % row_slices of its rows only — d / row_slices columns of X, addend,
                                       p, m, v, Y and S — so one XCD's L2 sees 1 / row_slices of every gathered row and holds
                                       row_slices times as many; the workgroups of a slice share the row tiles alternately.  A
                                       workgroup stages the row pointers and (col, val) entries of a tile of consecutive rows in
                                       LDS once and sorts the tile's rows by length; each output row is still summed by ONE
                                       sub-group in list order: bitwise the result of row_slices = 0.  A hint for speed: applies to
                                       planned launches without row_list (dense, addend_map, x_map, adam) whose d / 4 is a
                                       multiple of row_slices and whose plan->chunk fits the staging buffer (2048 entries);
                                       ignored elsewhere. */
    int32_t        slice_rows;      /* with row_slices: > 0 = only rows [0, slice_rows) run in the sliced form, the rows behind them
                                       in the plain one (a [users; items] adjacency: the item rows are long and gather from the
                                       user table, which has no popular part); 0 = all rows; < 0 is MI_ERR_BAD_ARG */
    const mi_spmm_tiles* tiles;     /* nullable (and null in a zero-initialised struct): the plan's hub rows run in TILES form, see
                                       mi_spmm_tiles; the plan's n_items then counts n_wg * n_slots partial rows in front of the
                                       work items'.  Not with x_map, row_list or a sweep (MI_ERR_BAD_ARG); d > 128, or an LDS size
                                       the device refuses: MI_ERR_UNSUPPORTED, returned BEFORE anything is enqueued when the call
                                       computes the split rows (parts = 0 or MI_SPMM_SPLIT_ROWS): relaunch with the adjacency's
                                       plan without tiles */
} mi_spmm_ex;
#define MI_SPMM_SHORT_ROWS 1
#define MI_SPMM_SPLIT_ROWS 2

int mi_spmm_csr_ex_f32(int64_t n_rows, int64_t d,
                       const int32_t* rowptr, const int32_t* col, const float* val,
                       const float* X, int64_t ldx,
                       float* Y, int64_t ldy,
                       const float* addend, int64_t lda,
                       float* S, int64_t lds, float scale,
                       const mi_spmm_plan* plan, const mi_spmm_ex* ex,
                       void* ws, size_t ws_bytes, mi_stream_t stream);

/* bits[w] bit b = (map[32 w + b] >= 0), w < ceil(n / 32): mi_spmm_ex.x_bits of a map. */
int mi_map_live_bits_i32(int64_t n, const int32_t* map, uint32_t* bits, mi_stream_t stream);

/* dst[i,:] = scale * ((accumulate ? dst[i,:] : 0) + src[rows[i] - row_offset,:])
 * for i in [begin_dev ? *begin_dev : 0, min(n_max, n_dev ? *n_dev : n_max)).
 * The running layer sum of the batch rows in the fused step (model/lightgcn.py:67-68 restricted
 * to the rows the loss reads); begin / row_offset address the item part of a batch node list
 * against an item-only table in the sharded step. */
int mi_gather_rows_f32(int64_t n_max, const int32_t* n_dev, const int32_t* begin_dev, int64_t d,
                       const int32_t* rows, int64_t row_offset, const float* src, int64_t ld_src,
                       float* dst, int64_t ld_dst, int32_t accumulate, float scale,
                       mi_stream_t stream);

/* dst[rows[i] - row_offset,:] = src[i,:] for i in [begin, min(n_max, *n_dev)); rows distinct.
 * Expands the item part of the compact batch gradient into the dense item table that the sharded
 * step all-reduces. */
int mi_scatter_rows_f32(int64_t n_max, const int32_t* n_dev, const int32_t* begin_dev, int64_t d,
                        const int32_t* rows, int64_t row_offset, const float* src, int64_t ld_src,
                        float* dst, int64_t ld_dst, mi_stream_t stream);

/* Unique node set of a BPR batch: gmap int32[n_nodes] = compact slot of node r (slots ordered by
 * node id) or -1; nodes int32[>= 3*batch] = slot -> node; count = device int32[2]:
 * count[0] = unique nodes, count[1] = unique USER nodes (their slots come first).
 * Users are nodes [0, n_users), item i is node n_users + i.
 * mi_batch_nodes_i32 is mi_batch_nodes_ex_i32 (below) with n_neg = 1. */
size_t mi_batch_nodes_workspace_bytes(int64_t n_nodes);
int    mi_batch_nodes_i32(int64_t batch, int64_t n_users, int64_t n_nodes,
                          const int64_t* users, const int64_t* pos, const int64_t* neg,
                          int32_t* gmap, int32_t* nodes, int32_t* count,
                          void* ws, size_t ws_bytes, mi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * K9  mini-batch sampler: B positive edges with replacement + one structured negative
 *     each, entirely on device.
 * replaces: sample_mini_batch at data/lightgcn_loader.py:95-112
 *           (structured_negative_sampling over all E edges on the CPU, then
 *           random.choices(range(E), k=B)).
 * Edge e = Philox(seed, step, slot b) mod nnz of the *train* CSR (rows = users, cols =
 * item ids in [0, n_items)); the negative for edge e is drawn from [0, neg_range) by
 * Philox keyed on (seed, step, e) — the same edge drawn twice in one step gets the same
 * negative, as in the reference — and redrawn while it is a neighbour of the user
 * (binary search in the user's sorted CSR row).  `quirk_user_rows` is a bit mask:
 * bit 0 (MI_SAMPLE_KEY_COLLISION): also rejects negative 0 for user u if user u-1 has an edge to
 *   item `neg_range` (the reference's row*num_nodes+col key collision);
 * bit 1 (MI_SAMPLE_NO_SELF_LOOPS): also rejects the negative whose id equals the user's id —
 *   structured_negative_sampling(contains_neg_self_loops=False) as evaluation() calls it
 *   (run_pipeline_lightgcn.py:40-44) puts the keys i*num_nodes+i of all i < num_nodes into the
 *   rejection set; sample_mini_batch (data/lightgcn_loader.py:105) leaves the default, True.
 * row_of_edge int32[nnz] is the expanded row index (mi_csr_expand_rows).
 * edges_in_order != 0: slot b takes edge b of the CSR instead of a random one (batch <= nnz) —
 * one negative per edge of a split, as evaluation() does (run_pipeline_lightgcn.py:40-44).
 * Outputs int64[B] each (the reference's index dtype).
 * This entry is mi_sample_bpr_batch_ex with n_neg = 1 (below), kept for the boundary: same checks, same kernel.
 * ---------------------------------------------------------------------------------- */
#define MI_SAMPLE_KEY_COLLISION 1
#define MI_SAMPLE_NO_SELF_LOOPS 2
int mi_csr_expand_rows(int64_t n_rows, const int32_t* rowptr, int32_t* row_of_edge,
                       int64_t nnz, mi_stream_t stream);
int mi_sample_bpr_batch(int64_t batch, int64_t nnz,
                        const int32_t* rowptr, const int32_t* col,
                        const int32_t* row_of_edge,
                        int64_t neg_range, int32_t quirk_user_rows, int32_t edges_in_order,
                        uint64_t seed, uint64_t step,
                        int64_t* users, int64_t* pos, int64_t* neg,
                        mi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * a7+a8  fused batch gather + BPR loss forward/backward.
 * replaces: the six index_selects at run_pipeline_lightgcn.py:133-144 and bpr_loss at
 *           utils/metrics_lightgcn.py:9-45, and their autograd backward.
 *   x_b  = <u_b,p_b> - <u_b,n_b>          (rows of final_emb)
 *   loss = -mean_b softplus(x_b) + lambda * sum_b (|u0_b|^2+|p0_b|^2+|n0_b|^2)   (rows of e0)
 * final_emb / e0: [n_users + n_items, d] tables (item i is row n_users + i).
 * loss_out: device float[1], written (fixed-order reduction).
 * When g_final is non-null (dense [n, d], ALL ZERO on entry) the rows the batch touches are written with
 *   g_final[row,:] = g_scale * dL/dfinal[row,:]          (untouched rows stay zero)
 * and reg_w (float[n], zeroed by the caller; nullable) receives reg_w[row] = (occurrences of the
 * node in the batch) * 2*lambda*reg_scale, so that the L2 term's gradient is
 * reg_w[row] * e0[row,:] (applied by mi_adam_dense_f32 or by the caller).  The count is the length
 * of the node's run in the sorted reference list: one writer per entry, no atomics.
 * node_map (nullable, from mi_batch_nodes_i32): final_emb and g_final are then COMPACT
 * [count, d] tables addressed by node_map[node]; e0 and reg_w stay addressed by node id.
 * No float atomics on the gradient: the 3*batch row references are radix-sorted by row, summed in
 * 64-reference chunks in reference order and combined in chunk order, one writer per row — the
 * result is bitwise reproducible.  d <= 512, with or without g_final (MI_ERR_UNSUPPORTED beyond).
 * This entry is the (MI_RANK_REFERENCE, n_neg = 1) case of mi_rank_loss_fwd_bwd_f32 (below), kept for the
 * boundary: the same host path, kernels and bits, and mi_bpr_workspace_bytes(b) ==
 * mi_rank_loss_workspace_bytes(b, 1).
 * ---------------------------------------------------------------------------------- */
size_t mi_bpr_workspace_bytes(int64_t batch);
int    mi_bpr_fwd_bwd_f32(int64_t batch, int64_t d, int64_t n_users,
                          const int64_t* users, const int64_t* pos, const int64_t* neg,
                          const float* final_emb, int64_t ldf,
                          const float* e0, int64_t lde,
                          float lambda, float g_scale, float reg_scale,
                          float* loss_out,
                          float* g_final, int64_t ldg,
                          float* reg_w,
                          const int32_t* node_map,
                          void* ws, size_t ws_bytes, mi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Ranking objectives over M negatives per positive (SURVEY F9 behind a flag).
 * A batch is users[B], pos[B], neg[B, n_neg] (int64, row-major), 1 <= n_neg <= 16; n_neg outside that range or
 * an unknown objective returns MI_ERR_UNSUPPORTED before anything is enqueued.
 *
 * Sampler: n_neg structured negatives per slot, drawn independently (they may repeat), same rejection rules and
 * quirk bits as the one-negative sampler.  Negative m of edge e, attempt t, takes the Philox counter
 * (e, t | m << 16) of the negative stream: column 0 is bit-identical to the one-negative sampler's output.
 *
 * Node set: the unique nodes over the (2 + n_neg) * batch references; same slot order contract and workspace as
 * the one-negative form; nodes int32[>= (2 + n_neg) * batch].
 *
 * Loss, with s+_b = <f_u, f_p>, s-_{b,m} = <f_u, f_{n_m}> on rows of final_emb and x_{b,m} = s+_b - s-_{b,m}:
 *   MI_RANK_REFERENCE  -(1/(B M)) sum softplus(x)      (torch softplus, threshold 20: the reference's objective)
 *   MI_RANK_BPR         (1/(B M)) sum softplus(-x)     = -mean log sigmoid(x)
 *   MI_RANK_SOFTMAX     (1/B) sum_b [ logsumexp(s+_b, s-_{b,1..M}) - s+_b ]   (max subtracted, m ascending)
 * plus lambda * sum_b (|u0|^2 + |p0|^2 + sum_m |n0_m|^2) on rows of e0.  reg_scale scales reg_w (the L2 term's
 * GRADIENT) only: the L2 term of the loss VALUE carries lambda alone, exactly as mi_bpr_fwd_bwd_f32 writes it, which the
 * bitwise identity at (MI_RANK_REFERENCE, n_neg = 1) needs for every reg_scale.
 * g_final, reg_w, node_map, g_scale, reg_scale, loss_out and the workspace behave as in the one-negative
 * entry: g_final[row] = g_scale * dL/dfinal[row] on zeroed input, reg_w[row] = occurrences * 2*lambda*reg_scale.
 * No float atomics on the gradient: the (2 + M) B row references (role 0 user, 1 positive, 2 + m negative m) are
 * stable-sorted by row and summed in 64-reference chunks in reference order, one writer per row — bitwise
 * reproducible.  d <= 512.  With MI_RANK_REFERENCE and n_neg = 1 loss, g_final and reg_w carry the bits of
 * the one-negative entry.
 * ---------------------------------------------------------------------------------- */
#define MI_RANK_REFERENCE 0
#define MI_RANK_BPR       1
#define MI_RANK_SOFTMAX   2
int mi_sample_bpr_batch_ex(int64_t batch, int32_t n_neg, int64_t nnz,
                           const int32_t* rowptr, const int32_t* col,
                           const int32_t* row_of_edge,
                           int64_t neg_range, int32_t quirk_user_rows, int32_t edges_in_order,
                           uint64_t seed, uint64_t step,
                           int64_t* users, int64_t* pos, int64_t* neg /* [batch, n_neg] */,
                           mi_stream_t stream);
int mi_batch_nodes_ex_i32(int64_t batch, int32_t n_neg, int64_t n_users, int64_t n_nodes,
                          const int64_t* users, const int64_t* pos, const int64_t* neg,
                          int32_t* gmap, int32_t* nodes, int32_t* count,
                          void* ws, size_t ws_bytes, mi_stream_t stream);
size_t mi_rank_loss_workspace_bytes(int64_t batch, int32_t n_neg);
int    mi_rank_loss_fwd_bwd_f32(int64_t batch, int32_t n_neg, int32_t objective, int64_t d, int64_t n_users,
                                const int64_t* users, const int64_t* pos, const int64_t* neg,
                                const float* final_emb, int64_t ldf,
                                const float* e0, int64_t lde,
                                float lambda, float g_scale, float reg_scale,
                                float* loss_out,
                                float* g_final, int64_t ldg,
                                float* reg_w,
                                const int32_t* node_map,
                                void* ws, size_t ws_bytes, mi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Popularity-weighted negatives and the logQ-corrected sampled softmax (SURVEY F9 behind a flag).
 *
 * Table (built once on the host in float64; ops.negative_table): with deg_i item i's degree in the TRAINING
 * interactions and 0 <= power <= 1,
 *   w_i    = deg_i ** power for deg_i > 0, else 0;     S = sum_i w_i  (float64, index order)
 *   q_i    = 0 if deg_i == 0, else max(1, floor(w_i / S * 2^31))
 *   cum[i] = q_0 + ... + q_i  (uint32);  total = cum[n_items - 1] < 2^32 for every n_items < 2^31
 *   logq[i] = float32(log(max(q_i, 1) / total)), the logarithm taken in float64 — an item of weight 0 gets the value
 *             of weight 1, so that a caller-supplied batch that names such an item stays finite.
 *
 * Draw (mi_sample_bpr_batch_pop): the counters of mi_sample_bpr_batch_ex, so the edge stream — users and pos — is
 * bit-identical to the uniform sampler's at the same (seed, step).  Negative m of edge e, attempt t, takes the Philox
 * counter (e, t | m << 16) of the negative stream, words (c0, c1, ..):
 *   r    = ((c0 << 32) | c1) % total
 *   cand = the smallest i with cum[i] > r   (bisection over cum in global memory; an item of weight 0 is never it)
 * redrawn while cand is one of the user's items, for at most the 4096 attempts of the other samplers; the last
 * candidate stays.  No quirk bits.  edges_in_order as in mi_sample_bpr_batch.  total is read from cum[n_items - 1] on
 * the device (no host wait); a zero total writes negative 0 for every slot.  One thread per (slot, m), one writer per
 * output, no atomics: two calls give equal bits.
 * Checked before any launch: MI_ERR_UNSUPPORTED for n_neg > 16; MI_ERR_BAD_ARG for null or misaligned pointers
 * (4 bytes for the int32 / uint32 arrays, 8 for the outputs) and for batch, n_neg, nnz or n_items below 1;
 * MI_ERR_TOO_LARGE for n_items >= 2^31 (and nnz >= 2^31 - 1, as in the other samplers).
 *
 * Loss (mi_rank_loss_fwd_bwd_lq_f32): mi_rank_loss_fwd_bwd_f32 plus logq float[n_items] (nullable), addressed by item
 * id whatever node_map is.  With logq, MI_RANK_SOFTMAX takes the logits
 *   s+_b - logq[pos_b]   and   s-_{b,m} - logq[neg_{b,m}]
 * in place of the raw scores: one fp32 subtraction each, applied after the wave sums; max subtraction, ascending-m
 * sum and coefficient formulas unchanged (the correction is a constant per logit, so the gradient keeps its form).
 * This makes the sampled softmax an estimate of the full softmax under the proposal q instead of penalising popular
 * items twice.  The rejection of the user's own items is NOT reflected in logq — the usual approximation.
 * logq == NULL: the kernels and the bits of mi_rank_loss_fwd_bwd_f32.  logq != NULL with another objective, or with
 * the loss-only form that accumulates reg_w (g_final == NULL, reg_w != NULL: the one path with float atomics), returns
 * MI_ERR_UNSUPPORTED before anything is enqueued.  Workspace: mi_rank_loss_workspace_bytes.
 * ---------------------------------------------------------------------------------- */
int mi_sample_bpr_batch_pop(int64_t batch, int32_t n_neg, int64_t nnz,
                            const int32_t* rowptr, const int32_t* col,
                            const int32_t* row_of_edge,
                            int64_t n_items, const uint32_t* cum /* [n_items] */, int32_t edges_in_order,
                            uint64_t seed, uint64_t step,
                            int64_t* users, int64_t* pos, int64_t* neg /* [batch, n_neg] */,
                            mi_stream_t stream);
int mi_rank_loss_fwd_bwd_lq_f32(int64_t batch, int32_t n_neg, int32_t objective, int64_t d, int64_t n_users,
                                const int64_t* users, const int64_t* pos, const int64_t* neg,
                                const float* final_emb, int64_t ldf,
                                const float* e0, int64_t lde,
                                float lambda, float g_scale, float reg_scale,
                                float* loss_out,
                                float* g_final, int64_t ldg,
                                float* reg_w,
                                const int32_t* node_map,
                                const float* logq /* [n_items], nullable */,
                                void* ws, size_t ws_bytes, mi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * In-batch sampled softmax (SURVEY F9 behind a flag): the other positives of the batch are every slot's negatives,
 * scored on the exact-f32 matrix instruction.  No negative is drawn and the node set is the 2 * batch references.
 *
 * A batch is users[B], pos[B] (int64); no neg.  group = G, a multiple of 32 with 32 <= G <= 4096.
 *   group g holds the slots [g*G, min((g+1)*G, B)): the last one may be partial, down to a single slot;
 *   the candidates of slot b are the slots j of its own group, with the logit
 *     l[b,j] = <f[users_b], f[n_users + pos_j]> - logq[pos_j]
 *   (f a row of final_emb; logq float[n_items] by item id whatever node_map is, nullable: NULL subtracts nothing);
 *   a candidate j != b is MASKED (left out of the sum, coefficient 0) when pos_j == pos_b (the slot's own positive) or
 *   users_j == users_b (pos_j is then an item that user bought).  The user's OTHER items that happen to be in the group
 *   are not rejected, and the masks are not reflected in logq — the usual approximations, as for the popularity sampler.
 *   loss = (1/B) sum_b [ logsumexp_{j unmasked, incl. j = b} l[b,j] - l[b,b] ]
 *          + lambda * sum_b (|e0[users_b]|^2 + |e0[n_users + pos_b]|^2)
 *   with the maximum subtracted before the exponentials; a slot with no unmasked candidate besides itself adds 0.
 *   c[b,j] = g_scale/B * (softmax_b[j] - [j == b]) for unmasked j;
 *   dL/df[users_b] += sum_j c[b,j] f[n_users + pos_j];   dL/df[n_users + pos_j] += sum_b c[b,j] f[users_b].
 * g_final, reg_w, node_map, g_scale, reg_scale and loss_out behave as in mi_rank_loss_fwd_bwd_f32: g_final all zero on
 * entry, only touched rows written; reg_w[row] = (occurrences among the 2B references) * 2*lambda*reg_scale; reg_scale does
 * not scale the L2 term of the loss VALUE.  The loss-only form is g_final == NULL and needs reg_w == NULL
 * (MI_ERR_UNSUPPORTED otherwise).  d % 4 == 0 and d <= 256 (MI_ERR_UNSUPPORTED otherwise).  final_emb, e0 and ws 16-byte
 * aligned, ldf and lde multiples of 4.  Every check — null or misaligned pointers, batch < 1, group, d, workspace — is made
 * before anything is enqueued.
 * The scores never reach memory: each pass (row statistics, the two gradient sweeps) recomputes its 32 x 32 score tiles
 * in the same k order, so all three see the same bits.  No float atomics: per-slot gradient rows, one writer each, are
 * summed per node by the sorted-reference segmented sum of the other losses (role 0 user, 1 positive).  Every order of
 * summation is a function of (B, G, d) and the ids only: two calls give equal bits.
 * mi_inbatch_softmax_workspace_bytes: 0 for arguments outside these limits.
 * ---------------------------------------------------------------------------------- */
size_t mi_inbatch_softmax_workspace_bytes(int64_t batch, int64_t d, int32_t group);
int    mi_inbatch_softmax_fwd_bwd_f32(int64_t batch, int32_t group, int64_t d, int64_t n_users,
                                      const int64_t* users, const int64_t* pos,
                                      const float* final_emb, int64_t ldf,
                                      const float* e0, int64_t lde,
                                      float lambda, float g_scale, float reg_scale,
                                      float* loss_out,
                                      float* g_final, int64_t ldg,
                                      float* reg_w,
                                      const int32_t* node_map,
                                      const float* logq /* [n_items], nullable */,
                                      void* ws, size_t ws_bytes, mi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Full-catalogue softmax (behind a flag): the objective the sampled softmaxes above estimate, computed exactly.  Every item
 * is a candidate of every slot; nothing is drawn, nothing is masked, nothing is corrected.
 *
 * A batch is users[B], pos[B] (int64); no neg.  f is a row of final_emb, whose user rows are [0, n_users) and whose item
 * rows are [n_users, n_users + n_items):
 *   l[b,i]  = <f[users_b], f[n_users + i]>                  for every i in [0, n_items)  — no mask, no logq
 *   loss    = (1/B) sum_b [ logsumexp_i l[b,i] - l[b,pos_b] ]
 *             + lambda * sum_b (|e0[users_b]|^2 + |e0[n_users + pos_b]|^2)
 *   with the maximum subtracted before the exponentials; n_items == 1 gives a main term of exactly 0 and zero gradients.
 *   c[b,i]  = g_scale/B * (softmax_b[i] - [i == pos_b])
 *   dL/df[users_b]      += sum_i c[b,i] f[n_users + i]
 *   dL/df[n_users + i]   = sum_b c[b,i] f[users_b]
 * g_final all zero on entry; on return EVERY item row holds its sum, the user rows the batch names hold theirs, other user
 * rows stay zero.  There is no node_map: this gradient is dense over the items, so the compact tables of a sparse batch do
 * not apply.  reg_w (zero on entry), g_scale, reg_scale and loss_out behave as in mi_inbatch_softmax_fwd_bwd_f32:
 * reg_w[row] = (occurrences among the 2B references) * 2*lambda*reg_scale; reg_scale does not scale the loss VALUE.  The
 * loss-only form is g_final == NULL and needs reg_w == NULL (MI_ERR_UNSUPPORTED otherwise).
 * d % 4 == 0 and 4 <= d <= 256 (MI_ERR_UNSUPPORTED otherwise); batch >= 1, 2 * batch < 2^31, 1 <= n_items < 2^31
 * (MI_ERR_TOO_LARGE past 2^31).  final_emb, e0 and ws 16-byte aligned, ldf and lde multiples of 4.  Every check is made
 * before anything is enqueued.
 * The scores never reach memory: the row statistics, the user-gradient sweep and the item-gradient sweep each recompute their
 * 32 x 32 score tiles through one routine in one k order, so all see the same bits.  No float atomics: an item row has one
 * writer for the whole pass over the batch; the per-slot user rows are summed per user by the sorted-reference segmented
 * sum of the other losses.  The catalogue is cut into item chunks whose (max, sum) pairs and partial user rows are merged in
 * ascending chunk order; the cut and every order of summation are functions of (B, n_items, d) and the ids only, not of the
 * device's size or of timing: two calls give equal bits, on any gfx950.  The workspace holds row images and per-chunk
 * partials, never anything of size B x n_items.
 * mi_full_softmax_workspace_bytes: 0 for arguments outside these limits.
 * ---------------------------------------------------------------------------------- */
size_t mi_full_softmax_workspace_bytes(int64_t batch, int64_t d, int64_t n_items);
int    mi_full_softmax_fwd_bwd_f32(int64_t batch, int64_t d, int64_t n_users, int64_t n_items,
                                   const int64_t* users, const int64_t* pos,
                                   const float* final_emb, int64_t ldf,
                                   const float* e0, int64_t lde,
                                   float lambda, float g_scale, float reg_scale,
                                   float* loss_out,
                                   float* g_final, int64_t ldg,
                                   float* reg_w,
                                   void* ws, size_t ws_bytes, mi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Noise-view contrastive term (behind a flag; XSimGCL, Yu et al., TKDE 2023, on the LightGCN backbone): every propagated
 * layer of ONE forward pass is perturbed by a small random vector, and the final read-out of a node is contrasted with the
 * same node's layer-l* embedding.  The perturbation is an additive constant (sign has zero derivative), so the backward is
 * the A^T chain of the unperturbed step with one more addend at layer l*.
 *
 * Perturbed propagate, for layer k = 1..K, Y_k = A X_{k-1} (X_0 = E0, the table):
 *   w       = Philox4x32-10( counter (id, c / 4, k, 0x58434C31), key (lo32(s), hi32(s)) ), s = seed + 0x9E3779B97F4A7C15 * step
 *             mod 2^64; id = the low 32 bits of the row's ORIGINAL id (row_ids[r], or r itself when row_ids is NULL); word
 *             c % 4 of the block belongs to column c
 *   u[r,c]  = (w >> 8) * 2^-24                        exact in fp32, in [0, 1)
 *   n[r,:]  = u[r,:] / max(|u[r,:]|_2, 1e-12)         the summation order of the norm is the kernel's own
 *   X_k[r,c] = Y_k[r,c] + eps * sign(Y_k[r,c]) * n[r,c]      sign(+-0) = 0: an all-zero row stays zero
 *   F = (1 / (K+1)) * sum_{k=0..K} X_k                (layer 0 is not perturbed)
 * A row's noise depends on (seed, step, k, id, c) only: not on n_rows, not on the leading dimension, not on the order of
 * the rows.  mi_perturb_rows_f32 perturbs x [n_rows, d] in place and, when S is given, also writes
 * S = (addend + X) * scale (addend nullable: zero; S may alias addend when lda == lds; neither may alias x), the running
 * layer sum of mi_spmm_csr_f32's epilogue.  d % 4 == 0 and 4 <= d <= 256 (MI_ERR_UNSUPPORTED otherwise); x, addend, S 16-byte
 * aligned, leading dimensions multiples of 4; eps >= 0, layer >= 0; n_rows == 0 is a no-op.  Every check is made before
 * anything is enqueued.  No atomics, one writer per element: two calls give equal bits.
 *
 * Contrast (mi_contrastive_fwd_bwd_f32), over ids[B] (int64 rows of BOTH tables a and b; the trainer calls it once with the
 * batch's users and once with its positives' node ids, a = F, b = X_{l*}), in groups of G consecutive slots as the in-batch
 * softmax cuts them (G a multiple of 32 in 32..4096, the last group may be partial):
 *   p_b = a[id_b] / max(|a[id_b]|, 1e-12)       q_b = b[id_b] / max(|b[id_b]|, 1e-12)
 *   l[b,j] = <p_b, q_j> * inv_tau               j in b's group; j != b is MASKED when id_j == id_b (the same node again)
 *   loss = (1/B) sum_b [ logsumexp_{j unmasked, incl. j = b} l[b,j] - l[b,b] ]
 * with the maximum subtracted before the exponentials; a slot alone in its group adds 0.  The contrast runs over slots, not
 * over distinct nodes: a node named m times weighs m times and its copies are masked as candidates of each other.
 *   g_a[id_b] += g_scale_a * dloss/da[id_b],  g_b[id_b] += g_scale_b * dloss/db[id_b], through the normalisation,
 *   dp/df = (I - p p^T) / |f| (a row under the 1e-12 floor: I / 1e-12).  The call ADDS to what the rows hold (it runs after
 *   the main loss, whose kernels demand zeros); rows that ids does not name are not touched.  The loss-only form is
 *   g_a == g_b == NULL; exactly one of them NULL is MI_ERR_UNSUPPORTED.  loss_out is written, not added to.
 * Limits and checks of mi_inbatch_softmax_fwd_bwd_f32: d % 4 == 0 and d <= 256 (MI_ERR_UNSUPPORTED), batch >= 1,
 * 2 * batch < 2^31 (MI_ERR_TOO_LARGE), ids < 2^31, inv_tau > 0 and finite, a, b and ws 16-byte aligned, lda and ldb multiples
 * of 4; all made before anything is enqueued.
 * The step (LightGCNTrainer, cl_weight > 0): loss = main loss + cl_weight * (L_user + L_item), L_user over id_b = users_b,
 * L_item over id_b = n_users + pos_b.  With gc = dL/dF / (K+1) (both terms) and G = cl_weight * dL_cl/dX_{l*}:
 *   h_K = gc (+ G if l* == K);   h_k = gc + A^T h_{k+1} (+ G if k == l*), k = K-1..1;   h_0 = gc + A^T h_1 = dL/dE0.
 * The call is the in-batch softmax's tile routine, row statistics and gradient sweeps on two normalised [B, d] images (p / tau
 * and q); the per-slot gradient rows go through the normalisation and are summed per id, in slot order, by the
 * sorted-reference segmented sum: one writer per row, no float atomics, two calls give equal bits.
 * mi_contrastive_workspace_bytes: 0 for arguments outside these limits.
 * ---------------------------------------------------------------------------------- */
int    mi_perturb_rows_f32(int64_t n_rows, int64_t d, float* x, int64_t ldx,
                           const int64_t* row_ids /* [n_rows], nullable */,
                           float eps, int32_t layer, uint64_t seed, uint64_t step,
                           const float* addend, int64_t lda, float* S, int64_t lds, float scale,
                           mi_stream_t stream);
size_t mi_contrastive_workspace_bytes(int64_t batch, int64_t d, int32_t group);
int    mi_contrastive_fwd_bwd_f32(int64_t batch, int32_t group, int64_t d, const int64_t* ids,
                                  const float* a, int64_t lda, const float* b, int64_t ldb,
                                  float inv_tau, float* loss_out,
                                  float* g_a, int64_t ldga, float g_scale_a,
                                  float* g_b, int64_t ldgb, float g_scale_b,
                                  void* ws, size_t ws_bytes, mi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * a9  dense Adam step (torch.optim.Adam semantics, no weight decay, no amsgrad).
 * replaces: optimizer.step() at run_pipeline_lightgcn.py:159.
 *   g   = grad[i] + (reg_w ? reg_w[row(i)] * p[i] : 0)
 *   m   = b1*m + (1-b1)*g ; v = b2*v + (1-b2)*g*g
 *   p  -= (lr / (1 - b1^step)) * m / (sqrt(v)/sqrt(1 - b2^step) + eps)
 * Hyper-parameters arrive as doubles and the derived scalars are formed in double on the
 * host before one rounding to fp32, as torch does; `step` counts from 1.
 * n_rows x d row-major, ld in floats; m, v dense [n_rows, d].
 * ---------------------------------------------------------------------------------- */
int mi_adam_dense_f32(int64_t n_rows, int64_t d,
                      float* p, int64_t ldp, const float* grad, int64_t ldgr,
                      float* m, float* v, const float* reg_w,
                      double lr, double beta1, double beta2, double eps, int64_t step,
                      mi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * K6  dense fp32 GEMM on the f32 MFMA (exact fp32, k-ordered fma chain):
 *   C[m,n] = act( sum_k A[m,k] * B(k,n) + bias[n] + (accumulate ? C[m,n] : 0) )
 * replaces: torch.nn.Linear inside SAGEConv (lin_l, lin_r) and the decoder MLP
 *           (model/layers.py:35-56, model/encoder_decoder.py:55-72) and their backward.
 * trans_a: A is stored [k,m] (lda = m-stride);  trans_b: B is stored [n,k] (the
 * nn.Linear weight layout).  act: 0 = none, 1 = relu.
 * Per output element the sum is one k-ascending fma chain (bitwise = oracle/spmm_ref.c), except
 * when the output grid is too small to fill the chip and k >= 2048 (weight gradients
 * dW = dY^T X): then, if the caller passes the workspace mi_gemm_workspace_bytes asks for, K is
 * cut into slices whose chains are added in a fixed association (still deterministic).  ws may be null.
 * ---------------------------------------------------------------------------------- */
size_t mi_gemm_workspace_bytes(int64_t m, int64_t n, int64_t k);
int    mi_gemm_f32(int32_t trans_a, int32_t trans_b, int64_t m, int64_t n, int64_t k,
                   const float* A, int64_t lda, const float* B, int64_t ldb,
                   const float* bias, float* C, int64_t ldc,
                   int32_t accumulate, int32_t act, void* ws, size_t ws_bytes, mi_stream_t stream);

/* Grouped form: any number of independent products, one launch per 8 (the ranker's per-batch products are
 * launch-bound, see csrc/gemm.hip).  Problem i:
 *     C = act( A @ B  [+ A2 @ B2]  + bias + (accumulate ? C : 0) )
 * with op(A) [m, k], op(B) [k, n] as in mi_gemm_f32 and an optional second pair sharing m, n and the trans flags
 * (k2 = 0: none) — lin_l(agg) + lin_r(x_dst) of SAGEConv (model/layers.py:11-24) as ONE product.  a_mask (nullable):
 * same storage layout as A; A's element is read as 0 where the mask element is <= 0 — the backward of a relu fused
 * into the producing product.  Operands must be float4-addressable (leading dimensions and k multiples of 4, 16-byte
 * aligned bases); otherwise MI_ERR_UNSUPPORTED — for the whole call, before anything is enqueued, whichever problem it is —
 * and the caller uses mi_gemm_f32.  Long-k / tiny-output problems are
 * split over k like mi_gemm_f32 (same slice rule, one grouped reduce).  ws: mi_gemm_group_workspace_bytes(). */
typedef struct mi_gemm_problem {
    int32_t trans_a, trans_b;
    int64_t m, n, k;
    const float* A; int64_t lda;
    const float* B; int64_t ldb;
    int64_t k2;
    const float* A2; int64_t lda2;
    const float* B2; int64_t ldb2;
    const float* a_mask;
    const float* bias;
    float* C; int64_t ldc;
    int32_t accumulate, act;
} mi_gemm_problem;
size_t mi_gemm_group_workspace_bytes(const mi_gemm_problem* problems, int32_t n);
int mi_gemm_group_f32(const mi_gemm_problem* problems, int32_t n, void* ws, size_t ws_bytes, mi_stream_t stream);
/* 1 when mi_gemm_group_f32 would take every problem (float4-addressable operands), 0 when it would return
 * MI_ERR_UNSUPPORTED; enqueues nothing. */
int mi_gemm_group_supported(const mi_gemm_problem* problems, int32_t n);

/* What mi_gemm_f32 will do with these arguments; host-only, enqueues nothing (the precedent is mi_topk_path).  The launcher asks
 * the same function, so the answer is what runs.  A and B are tested for alignment only, never read.  a_gathered != 0: A's rows
 * come through a row map (the score products of K10; mi_gemm_f32 itself passes none).  ws_bytes: the workspace the call will
 * get, 0 for none.
 *
 *   kernel    chosen when
 *   KK KR     both operands float4-addressable: 16-byte aligned bases; a K-contiguous operand (A without trans_a, B with
 *   RK RR     trans_b) has ld % 4 == 0, a row-contiguous one ld % 4 == 0 and no row map; k % 4 == 0 unless BOTH are
 *             row-contiguous.  First letter A, second B: K = K-contiguous, R = row-contiguous.
 *   GENERIC   everything else
 *   NONE      m == 0 or n == 0: nothing is launched (splits = 0)
 *
 * splits / k_per_split: with T = ceil(m / 64) * ceil(n / 64) output tiles, K is cut when T <= 8 and k >= 512 (at least 128 of K
 * per slice) or 9 <= T <= 127 and k >= 2048 (at least 256 per slice), and the workspace holds the slabs:
 * s = min(ceil(512 / T), k / 128 or k / 256); k_per_split = ceil(k / s) rounded up to 32; splits = ceil(k / k_per_split).
 * Otherwise splits = 1, k_per_split = k.
 * Returns 0, or the negative code mi_gemm_f32 would return for these arguments: MI_ERR_BAD_ARG (a negative size, a null out or
 * operand, a leading dimension below the operand's width), MI_ERR_TOO_LARGE (more than 65 535 row tiles). */
#define MI_GEMM_KERNEL_NONE    (-1)
#define MI_GEMM_KERNEL_GENERIC 0  /* gemm_f32_kernel                */
#define MI_GEMM_KERNEL_FAST_KK 1  /* gemm_fast_kernel<true, true>   */
#define MI_GEMM_KERNEL_FAST_KR 2  /* gemm_fast_kernel<true, false>  */
#define MI_GEMM_KERNEL_FAST_RK 3  /* gemm_fast_kernel<false, true>  */
#define MI_GEMM_KERNEL_FAST_RR 4  /* gemm_fast_kernel<false, false> */
typedef struct mi_gemm_plan_info {
    int32_t kernel, splits;
    int64_t k_per_split;
} mi_gemm_plan_info;
int mi_gemm_plan(int32_t trans_a, int32_t trans_b, int64_t m, int64_t n, int64_t k,
                 const float* A, int64_t lda, const float* B, int64_t ldb,
                 int32_t a_gathered, size_t ws_bytes, mi_gemm_plan_info* out);

/* The layout mi_gemm_group_f32 gives these problems (workspace assumed sufficient); host-only, enqueues nothing; it is the
 * launch's own layout pass.  out[i] for problem i: `launch` = which launch of 8 it rides in; splits / k_per_split as run (a
 * two-pair problem is never split; a K-contiguous operand keeps k_per_split a multiple of 4); share_set = index, within its
 * launch, of the share set it belongs to, -1 for none.  A share set is a run of >= 2 consecutive split single-pair problems
 * over the same A (pointer, k, strides, mask): all members get the coarsest member's k_per_split, and their workgroups are
 * laid slice-major from a multiple of 8 on, ceil(splits / 8) * 8 * (sum of the members' tiles) of them, the excess idle.
 * first_wg / n_wg: the problem's range of linear workgroups in its launch (a set's members all report the set's range; idle
 * workgroups that pad the start of a following set are not counted); an empty problem has splits = 0, n_wg = 0.
 * Returns MI_ERR_UNSUPPORTED / MI_ERR_BAD_ARG exactly where the launch would, before anything is laid out: a call is taken
 * whole or not at all. */
typedef struct mi_gemm_group_plan_info {
    int32_t launch, splits;
    int64_t k_per_split;
    int32_t share_set, reserved;
    int64_t first_wg, n_wg;
} mi_gemm_group_plan_info;
int mi_gemm_group_plan(const mi_gemm_problem* problems, int32_t n, mi_gemm_group_plan_info* out);

/* ------------------------------------------------------------------------------------
 * K10  batched exact top-K with per-user exclusion.
 * replaces: make_predictions_for_user at utils/metrics_lightgcn.py:125-142
 *           (scores = e_u @ E_i^T; topk(k+|ignore|); order-preserving setdiff; [:k]).
 * scores[u, i] = fmaf-chain over d ascending of user_emb[uid[u], :] . item_emb[i, :]
 * (bitwise equal to oracle/spmm_ref.c:ref_scores_fma_f32); excluded items (excl_ptr/excl_idx: CSR by
 * position in uid, item ids sorted or not) never appear; output int64[n_q, k] item ids
 * by descending score, ties by ascending item id; -1 pads when fewer than k remain.
 * k <= 1024.  For n_items >= 32 768 and d <= 128 (multiple of 4, 16-byte aligned tables) the score block is never
 * written: scores are compared in the MFMA epilogue with a per-row threshold taken from a 4 096-item sample and only the
 * survivors are kept; a row whose survivors are fewer than k or overflow its list recomputes its scores and takes
 * the exact multi-pass selection, so the result is the same as on the materialised path (smaller item sets).
 * For d = 64 / 128 and k <= 256 the candidates are picked by a bf16x3 PREFILTER (csrc/topk_prefilter.hpp): both tables
 * split into bf16 hi + lo parts, u_hi.i_hi + u_lo.i_hi + u_hi.i_lo on the bf16 MFMA, every score within a proven
 * eps(u) = 2^-12 |u| max|i| of the f32 chain; the items that can still reach the answer under that bound are scored
 * again with the exact fma chain and the answer is picked from those — ids and scores are the f32 path's bit for bit
 * (environment LAPLACE_TOPK_PREFILTER=0, read per call, selects the f32 fused kernel: A/B and tests of both; about 2.7 x
 * the f32 kernel's throughput: 10.6 M against 3.9 M users/s at k = 12, 100 K items, D = 128).
 * Workspace (mi_topk_workspace_bytes): address space for the [n_q, n_items] fp32 score block (touched only by
 * fallback rows on the fused path) + sample scores, exclusion bitmap, candidate lists, the split tables: callers chunk
 * n_q (multiples of 2 048 queries fill the prefilter's grid in whole rounds).
 * ---------------------------------------------------------------------------------- */
size_t mi_topk_workspace_bytes(int64_t n_q, int64_t n_items, int64_t k);
int    mi_topk_excl_f32(int64_t n_q, int64_t n_items, int64_t d, int64_t k,
                        const int64_t* uid,
                        const float* user_emb, int64_t ldu,
                        const float* item_emb, int64_t ldi,
                        const int32_t* excl_ptr, const int32_t* excl_idx,
                        int64_t* out_idx, float* out_score /* nullable */,
                        void* ws, size_t ws_bytes, mi_stream_t stream);
/* The same with flags.  MI_TOPK_ITEMS_PREPARED: `ws` still holds the ITEM side of the bf16 prefilter (the sampled item rows, the
 * bf16 hi / lo split of the item table and of the sample, the largest |item|^2) from the previous call on this stream with
 * the same item table, n_q, n_items, d and k — callers that cut one request into equal chunks of queries set it from the second
 * chunk on (one split of a 100 K-item table is ~40 us of a ~550 us chunk).  Ignored on the paths without a prefilter. */
#define MI_TOPK_ITEMS_PREPARED 1u
int    mi_topk_excl_ex_f32(int64_t n_q, int64_t n_items, int64_t d, int64_t k, const int64_t* uid,
                           const float* user_emb, int64_t ldu, const float* item_emb, int64_t ldi,
                           const int32_t* excl_ptr, const int32_t* excl_idx, int64_t* out_idx,
                           float* out_score, void* ws, size_t ws_bytes, uint32_t flags, mi_stream_t stream);

/* Which of K10's five code paths a call with these arguments takes; host-only, enqueues nothing (the precedent is
 * mi_gemm_group_supported).  The dispatcher of mi_topk_excl_ex_f32 asks the same function, so the answer is what runs.
 * "fused-eligible": n_items >= 32 768, d <= 128, d % 4 == 0, ldu % 4 == 0, ldi % 4 == 0, both bases 16-byte aligned.
 *
 *   path                       chosen when                                               select step
 *   M   materialised           n_items < 32 768                                          select_kernel, multi-pass
 *   M1  materialised, one pass n_items >= 32 768 and not fused-eligible                  select_kernel, sampled threshold
 *                                                                                        + one collect pass
 *   G   fused, generic         fused-eligible, d neither 64 nor 128                      topk_scores_filter_kernel; sample
 *                                                                                        scores from the plain GEMM
 *   D   fused, LDS-DMA         fused-eligible, d 64 or 128, and the prefilter is off,    topk_scores_filter_dma_kernel
 *                              k > 256, or the prefilter's LDS attribute is refused
 *   P   bf16x3 prefilter       fused-eligible, d 64 or 128, k <= 256, prefilter on       topk_prefilter_launch
 *                              and usable
 *
 * user_emb / item_emb are tested for alignment only, never read.  LAPLACE_TOPK_PREFILTER is read per call, as the
 * dispatcher reads it; the build switches MI_TOPK_FUSED, MI_TOPK_ONE_PASS and MI_TOPK_DMA are honoured, so an A/B build
 * reports what it runs.  Only a P answer touches the HIP runtime (the kernel's LDS attribute on the current device).
 * Bad arguments: the negative codes of mi_topk_excl_ex_f32 (MI_ERR_BAD_ARG, MI_ERR_UNSUPPORTED for k > 1024,
 * MI_ERR_TOO_LARGE).
 * NON-FINITE inputs (NaN / inf embeddings) are outside K10's contract on every path: the order of such scores is
 * unspecified. */
#define MI_TOPK_PATH_MATERIALISED 0 /* M  */
#define MI_TOPK_PATH_ONE_PASS     1 /* M1 */
#define MI_TOPK_PATH_FUSED        2 /* G  */
#define MI_TOPK_PATH_FUSED_DMA    3 /* D  */
#define MI_TOPK_PATH_PREFILTER    4 /* P  */
int mi_topk_path(int64_t n_items, int64_t d, int64_t k,
                 const float* user_emb, int64_t ldu,
                 const float* item_emb, int64_t ldi);

/* Diagnostic of K10's bf16x3 prefilter (csrc/topk_prefilter.hpp), d = 64 / 128: scores[q, i] = the APPROXIMATE score the
 * prefilter compares with its thresholds, eps[q] = the bound it assumes, |scores[q, i] - exact fma chain| <= eps[q] for
 * every item (tests/test_gpu_topk_gemm.py asserts it on adversarial tables).  Not on any product path: the candidates'
 * exact scores are what mi_topk_excl_f32 returns. */
size_t mi_topk_prefilter_scores_workspace_bytes(int64_t n_q, int64_t n_items);
int    mi_topk_prefilter_scores_f32(int64_t n_q, int64_t n_items, int64_t d,
                                    const int64_t* uid /* nullable */,
                                    const float* user_emb, int64_t ldu,
                                    const float* item_emb, int64_t ldi,
                                    float* scores /* [n_q, n_items] */, float* eps /* [n_q] */,
                                    void* ws, size_t ws_bytes, mi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * K10r  full-catalogue rank of one target item per query row (csrc/rank.hip).
 * The reference has no such call: it reads every metric off a top-k list (utils/metrics_lightgcn.py:79-122).  This is the
 * quantity behind MRR, mean rank, AUC, MAP and recall@K at any K: how many admissible items beat the held-out one.
 * For query row p with user uid[p], target t = target[p] and exclusion row excl(p) (excl_ptr / excl_idx: CSR by position
 * in uid, K10's contract: ids sorted or not, repeats allowed, ids outside [0, n_items) ignored):
 *   s_j      = fmaf-chain over d ascending, from 0, of user_emb[uid[p], :] . item_emb[j, :]   (K10's scores, bit for bit)
 *   key(s)   = score_key of csrc/score_panel.hpp (-0 -> +0, monotone)
 *   j BEATS t  iff  key(s_j) > key(s_t), or key(s_j) == key(s_t) and j < t                    (K10's order)
 *   rank[p]  = #{ j in [0, n_items) : j != t, j not in excl(p), j beats t }
 *   rank[p]  = -1 if t is in excl(p) or t is outside [0, n_items)
 *   score[p] = s_t (nullable output); 0 when t is outside [0, n_items)
 *   n_excluded[p] = number of DISTINCT in-range ids of excl(p) (nullable output; AUC's denominator needs it)
 * Hence for every k <= 1024: t stands in column c of mi_topk_excl_f32's row for the same user and exclusions iff
 * rank[p] == c < k.  uid may repeat: a user with five held-out items is five rows.  All outputs are integers or single
 * fma chains: exact, and equal from call to call.  NON-FINITE embeddings are outside the contract, as for K10.
 * Two paths, chosen by mi_rank_path's function:
 *   F  fused          d <= 128, d % 4 == 0, ldu % 4 == 0, ldi % 4 == 0, both bases 16-byte aligned (K10's "fused-eligible"
 *                     without its n_items >= 32 768: any n_items): scores on the f32 MFMA, compared and counted in
 *                     registers, never written; one integer atomicAdd per row and workgroup
 *   M  materialised   everything else: the [n_q, n_items] score block through the GEMM of K10's M path, one counting
 *                     workgroup per row
 * Exclusions on both paths: every item is counted first; one pass over a row's list then takes back the excluded items
 * that beat t (first occurrences found with a per-call bitmap in `ws`).
 * Errors: MI_ERR_BAD_ARG; MI_ERR_TOO_LARGE for n_items >= 2^31 - 1 or n_q > 65 535 * 64 (callers chunk n_q);
 * MI_ERR_WORKSPACE when ws_bytes < mi_rank_items_workspace_bytes(n_q, n_items): address space for path M's score block
 * (never touched on path F), n_q * n_items / 8 bytes of bitmap, 8 bytes per row.
 * ---------------------------------------------------------------------------------- */
size_t mi_rank_items_workspace_bytes(int64_t n_q, int64_t n_items);
int    mi_rank_items_f32(int64_t n_q, int64_t n_items, int64_t d,
                         const int64_t* uid, const int64_t* target /* int64[n_q] */,
                         const float* user_emb, int64_t ldu,
                         const float* item_emb, int64_t ldi,
                         const int32_t* excl_ptr /* nullable */, const int32_t* excl_idx,
                         int32_t* out_rank /* int32[n_q] */, float* out_score /* nullable */,
                         int32_t* out_n_excluded /* nullable int32[n_q] */,
                         void* ws, size_t ws_bytes, mi_stream_t stream);
/* Which path a call with these tables takes; host-only, enqueues nothing, the dispatcher's own decision function (the
 * precedent is mi_topk_path).  The pointers are tested for alignment only.  Negative: MI_ERR_BAD_ARG, MI_ERR_TOO_LARGE. */
#define MI_RANK_PATH_MATERIALISED 0 /* M */
#define MI_RANK_PATH_FUSED        1 /* F */
int mi_rank_path(int64_t n_items, int64_t d,
                 const float* user_emb, int64_t ldu,
                 const float* item_emb, int64_t ldi);

/* ------------------------------------------------------------------------------------
 * K5  SAGEConv message passing.
 * replaces: SAGEConv.propagate -> torch_scatter.scatter(x_j, index, reduce=aggr) reached from
 *           model/layers.py:11-24 via model/encoder_decoder.py:32,44.
 * The CSR is by DESTINATION node (rowptr over dst, col = source ids, sorted).
 *   aggr="add":  mi_spmm_csr_f32 with val = 1          (no [E, C] message tensor, no atomics)
 *   aggr="mean": mi_spmm_csr_f32 with val = 1/in-degree (mi_scale_csr_f32); empty segment -> 0
 *   aggr="max":  mi_segment_max_f32 below; empty segment -> 0; `arg` int32[n_dst, d] (nullable)
 *                receives the winning source id (-1 for empty) for the backward
 *                dX[s, c] = sum over destinations r of s with arg[r, c] == s of dY[r, c],
 *                computed per SOURCE row over the by-source CSR of the same relation (src_rowptr over
 *                sources, src_col = destination ids, sorted): one writer per element, fixed order,
 *                no float atomics; every row of dX is written.
 * ---------------------------------------------------------------------------------- */
int mi_segment_max_f32(int64_t n_dst, int64_t d, const int32_t* rowptr, const int32_t* col,
                       const float* X, int64_t ldx, float* Y, int64_t ldy, int32_t* arg,
                       mi_stream_t stream);
int mi_segment_max_bwd_f32(int64_t n_src, int64_t d, const int32_t* src_rowptr, const int32_t* src_col,
                           const int32_t* arg, const float* dY, int64_t ldy, float* dX, int64_t ldx,
                           mi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * K7  multi-column categorical embedding lookup + concat, with max_norm renorm.
 * replaces: Encoder_Decoder_Model.__embedding at model/encoder_decoder.py:116-125
 *           (Embedding(num_cat+1, size, max_norm=1)(x[:, i]) per column, cat on dim 1).
 * x int64[n, n_cols] (device).  tables / table_rows / dims are HOST arrays of n_cols (<= 16)
 * entries: device pointer to float[rows_c, dim_c], rows_c, dim_c.  out float[n, sum(dim_c)].
 * A looked-up row whose L2 norm exceeds max_norm is scaled by max_norm / (norm + 1e-7) on the
 * fly — the value torch's in-place embedding_renorm_ would leave in the table — so the stored
 * (frozen) table is never written.  max_norm <= 0 disables it.
 * ---------------------------------------------------------------------------------- */
int mi_embed_concat_f32(int64_t n, int32_t n_cols, const int64_t* x,
                        const float* const* tables, const int64_t* table_rows, const int32_t* dims,
                        float max_norm, float* out, int64_t ldo, mi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * K8  per-node-type BatchNorm1d over the nodes of a batch.
 * replaces: self.encoder_layer_norm_customer / _article = BatchNorm1d(out_channels) applied at
 *           model/encoder_decoder.py:144-150 (declared :98-99) and its autograd backward.
 * training != 0: batch statistics (biased variance for the normalisation; running_mean /
 * running_var updated in place with `momentum` and the UNBIASED variance, torch semantics;
 * pass both null to skip); save_mean / save_invstd float[c] are written for the backward.
 * training == 0: y = (x - running_mean) / sqrt(running_var + eps) * gamma + beta.
 * gamma / beta nullable (affine=False).  Backward: dX (nullable) and dgamma / dbeta (nullable)
 * from the saved statistics.  Sums are reduced in double in a fixed order: bitwise reproducible.
 * ws: mi_batchnorm_workspace_bytes(c) bytes, device.  c <= 512.
 * ---------------------------------------------------------------------------------- */
size_t mi_batchnorm_workspace_bytes(int64_t c);
int mi_batchnorm_fwd_f32(int64_t n, int64_t c, const float* X, int64_t ldx,
                         const float* gamma, const float* beta,
                         float* running_mean, float* running_var, float momentum, float eps,
                         int32_t training, float* save_mean, float* save_invstd,
                         float* Y, int64_t ldy, void* ws, size_t ws_bytes, mi_stream_t stream);
int mi_batchnorm_bwd_f32(int64_t n, int64_t c, const float* X, int64_t ldx,
                         const float* dY, int64_t ldy, const float* gamma,
                         const float* save_mean, const float* save_invstd,
                         float* dX, int64_t lddx, float* dgamma, float* dbeta,
                         void* ws, size_t ws_bytes, mi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * b9  the ranker's objective and its gradient in one launch.
 * replaces: torch.nn.BCEWithLogitsLoss()(logits, edge_label.float()) at training.py:26-31 and the backward of it.
 * loss[0] = mean(max(x,0) - x*y + log1p(exp(-|x|))); dlogits (nullable) = (sigmoid(x) - y) / n.  One workgroup,
 * double sums in a fixed tree.
 * ---------------------------------------------------------------------------------- */
int mi_bce_logits_f32(int64_t n, const float* logits, const float* labels, float* loss, float* dlogits,
                      mi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * b1  weight gradients of SAGEConv relations (model/layers.py:11-24: out = lin_l(AGG x_src) + lin_r(x_dst)):
 *   gw1 [m, n1] = (dy * relu')^T b1,   gb [m] = (dy * relu')^T 1 (nullable),   gw2 [m, n2] = (dy * relu')^T b2 (n2 = 0: none)
 * with dy [k, m] the gradient at the layer's output (k = destination nodes), mask [k, m] nullable (dy is read as 0 where
 * mask <= 0: the relu behind the layer), b1 = the aggregated source features [k, n1], b2 = the destination features [k, n2].
 * replaces: what autograd derives for the two Linear layers of torch_geometric.nn.SAGEConv (three transposed products).
 * All matrices dense row-major (leading dimension = width).  m a multiple of 32, <= 128; n1, n2 <= 512; up to 4 problems
 * per call (the two relations of a layer).  No LDS staging: rows of dy / b1 / b2 go straight into the operand registers
 * of the f32 32x32x2 MFMA; K is cut into slices whose partial outputs are summed in slice order (deterministic).
 * MI_ERR_UNSUPPORTED (nothing enqueued) for other shapes: callers use the grouped GEMM.
 * ---------------------------------------------------------------------------------- */
typedef struct mi_wgrad_problem {
    int64_t k;
    int32_t m, n1, n2, reserved;
    const float *dy, *mask, *b1, *b2;
    float *gw1, *gb, *gw2;
} mi_wgrad_problem;
int    mi_sage_wgrad_supported(const mi_wgrad_problem* problems, int32_t n);
size_t mi_sage_wgrad_workspace_bytes(const mi_wgrad_problem* problems, int32_t n);
int    mi_sage_wgrad_f32(const mi_wgrad_problem* problems, int32_t n, void* ws, size_t ws_bytes, mi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * b7  backward of a Linear layer with ONE output feature — the last decoder layer (model/encoder_decoder.py:66-72,
 * Linear(128, 1)): dx[r, :] = dy[r] * w (nullable), gw = sum_r dy[r] x[r, :], gb = sum_r dy[r] (nullable).
 * replaces: the three [n, 1]-shaped products autograd derives for that layer (torch.nn.Linear backward).
 * Deterministic (bands of 64 rows reduced in band order).  ws: mi_linear1_bwd_workspace_bytes(n, in).
 * ---------------------------------------------------------------------------------- */
size_t mi_linear1_bwd_workspace_bytes(int64_t n, int64_t in);
int    mi_linear1_bwd_f32(int64_t n, int64_t in, const float* dy, const float* w, const float* x, int64_t ldx,
                          float* dx, int64_t lddx, float* gw, float* gb, void* ws, size_t ws_bytes, mi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * b7  decoder input: z = cat(z_user[row], z_item[col], dim=-1) over the label edges.
 * replaces: EdgeDecoder.forward's two index_selects + cat at model/encoder_decoder.py:57-63
 *           and their backward (index_add into the two node tables).
 * out float[n_edges, cu + ci].  Backward, one call per node table: dZ[v, :] = sum over the
 * label edges e (ascending) with idx[e] == v of dOut[e, off : off + c]; dZ must be zero-filled
 * by the caller (rows no edge names stay zero).  One writer per row, fixed order, no atomics;
 * supports up to mi_gather_cat_bwd_max_edges() label edges (MI_ERR_UNSUPPORTED beyond).
 * ---------------------------------------------------------------------------------- */
int mi_gather_cat_f32(int64_t n_edges, int64_t cu, int64_t ci, const int64_t* row, const int64_t* col,
                      const float* Zu, int64_t ldu, const float* Zi, int64_t ldi,
                      float* out, int64_t ldo, mi_stream_t stream);
int64_t mi_gather_cat_bwd_max_edges(void);
int mi_gather_cat_bwd_f32(int64_t n_edges, int64_t c, int64_t off, const int64_t* idx,
                          const float* dOut, int64_t ldo, float* dZ, int64_t ldz, mi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * b9  native executor of ONE ranker training iteration (round 3).
 * replaces: the loop body of training.py:19-34 (`zero_grad -> model(...) -> BCEWithLogitsLoss -> backward ->
 *           optimizer.step`) for the model shape the reference builds by default (model/encoder_decoder.py:75-150,
 *           run_pipeline.py:47-73): two node types (customer, article) with categorical features and frozen embedding
 *           tables, the two relations customer -buys-> article and its reverse, L SAGEConv layers (add / mean) duplicated
 *           per relation, per-type BatchNorm1d, an MLP decoder over cat(z_customer[row], z_article[col]), Adam.
 * One call enqueues the whole iteration — the same mi_* launches, in the same order and with the same operands, as
 * the package's FusedRankerStep issues one by one from Python — so the host cost is one FFI call instead of ~75 op
 * calls.  Every buffer the iteration needs is carved from `ws` (mi_ranker_step_workspace_bytes); gradients are
 * written to the caller's persistent gradient buffers and consumed by a multi-tensor Adam launch (skippable:
 * data-parallel callers all-reduce the gradients first).  Feature dropout draws Philox4x32-10 masks keyed on
 * (seed, step, site) and regenerates them in the backward.  Returns MI_ERR_UNSUPPORTED (nothing enqueued) for shapes
 * outside the above; the caller then runs the op-by-op path.
 * ---------------------------------------------------------------------------------- */
#define MI_RANKER_MAX_LAYERS 4
#define MI_RANKER_MAX_COLS 16
#define MI_RANKER_MAX_PARAMS 48
typedef struct mi_ranker_conv {        /* SAGEConv of one relation in one layer: out = lin_l(AGG x_src) + lin_r(x_dst) */
    const float *w_l, *b_l, *w_r;      /* [c_out, c_src], [c_out] (nullable), [c_out, c_dst] */
    float *gw_l, *gb_l, *gw_r;         /* gradients, same shapes (gb_l nullable with b_l) */
    int32_t c_src, c_dst, c_out, reserved;
} mi_ranker_conv;
typedef struct mi_ranker_norm {        /* BatchNorm1d of one node type */
    const float *gamma, *beta;         /* nullable (affine=False) */
    float *running_mean, *running_var; /* nullable (track_running_stats=False) */
    int64_t* num_batches_tracked;      /* nullable; incremented by one */
    float *g_gamma, *g_beta;
    float momentum, eps;
} mi_ranker_norm;
typedef struct mi_ranker_linear {
    const float *w, *b;                /* [out, in], [out] (nullable) */
    float *gw, *gb;
    int32_t in, out;
} mi_ranker_linear;
typedef struct mi_ranker_param {       /* one tensor of the optimizer's parameter list */
    float *p, *g, *m, *v;
    int64_t n;
} mi_ranker_param;
typedef struct mi_ranker_model {
    int32_t n_enc_layers, n_dec_layers;
    int32_t aggr;                      /* 0 = add, 1 = mean */
    int32_t batch_normalize;
    float   p_dropout;                 /* feature dropout in front of every non-last encoder / decoder layer; 0 = none */
    float   max_norm;                  /* of the embedding lookups (reference: 1) */
    /* node type 0 = customer, 1 = article */
    int32_t n_cols[2];
    const float* tables[2][MI_RANKER_MAX_COLS];
    int64_t table_rows[2][MI_RANKER_MAX_COLS];
    int32_t dims[2][MI_RANKER_MAX_COLS];
    /* conv[l][0]: customer -> article (destination: article); conv[l][1]: article -> customer */
    mi_ranker_conv conv[MI_RANKER_MAX_LAYERS][2];
    mi_ranker_norm norm[2];
    mi_ranker_linear dec[MI_RANKER_MAX_LAYERS];
    int32_t n_params, apply_adam;      /* apply_adam = 0: stop after the gradients */
    mi_ranker_param params[MI_RANKER_MAX_PARAMS];
    double lr, beta1, beta2, eps;
    int64_t step;                      /* Adam step of THIS iteration, counts from 1 */
    const float* ones4;                /* device float[n_ones, 4] of ones (bias gradients ride in the grouped dW launch) */
    int64_t n_ones;
} mi_ranker_model;
typedef struct mi_ranker_batch {
    int64_t n_nodes[2];                /* customers, articles of the batch */
    const int64_t* x[2];               /* int64[n_nodes[t], n_cols[t]] categorical features */
    /* the batch's `buys` edges as two sorted CSRs (what mi_sampler_emit_csr writes) */
    const int32_t *by_customer_ptr, *by_customer_col;   /* rows = customers, columns = articles */
    const int32_t *by_article_ptr, *by_article_col;     /* rows = articles, columns = customers */
    int64_t nnz;
    int64_t n_label;
    const int64_t *label_row, *label_col;  /* customer / article index of every label edge */
    const int64_t* label;                  /* int64[n_label] 0 / 1 (the sampler's edge_label), or null when ... */
    uint64_t seed, step;                   /* dropout stream */
    float* loss;                           /* device float[1] */
    const float* label_f32;                /* ... the caller already holds the labels as float[n_label] */
    /* optional second stream: pairs of independent small launches (customer / article twins) then run side by side.
     * aux_stream: a hipStream_t; ev_fork / ev_join: two hipEvent_t (timing disabled) owned by the caller and used by no one
     * else while the call is in flight.  All three null = everything on `stream`.  Results do not depend on it. */
    void *aux_stream, *ev_fork, *ev_join;
    /* INFERENCE (round 4; model(x, edge_index, edge_label_index) under model.eval(): run_submission.py:55-58): non-null =
     * forward only, in evaluation mode — no dropout, BatchNorm with its running statistics (required) — and the decoder's
     * output per label edge goes to logits[n_label].  label / label_f32 / loss, every gradient pointer of the model and its
     * parameter list are then neither required nor read; nothing of the model is written. */
    float* logits;
} mi_ranker_batch;
int64_t mi_ranker_sizeof(int32_t which);  /* sizeof of: 0 model, 1 batch, 2 conv, 3 norm, 4 linear, 5 param (binding self-check) */
size_t mi_ranker_step_workspace_bytes(const mi_ranker_model* model, const mi_ranker_batch* batch);
int    mi_ranker_step_f32(const mi_ranker_model* model, const mi_ranker_batch* batch, void* ws, size_t ws_bytes,
                          mi_stream_t stream);
/* The validation pass of mi_ranker_step_f32 alone: 0 when the call would be taken, MI_ERR_UNSUPPORTED / MI_ERR_ARG when it
 * would be declined.  Enqueues nothing and reads no device memory (host-side walk of the two descriptors), so data-parallel
 * callers can agree on taking or declining a batch BEFORE any rank enters the gradient all-reduce (round 4). */
int    mi_ranker_step_check(const mi_ranker_model* model, const mi_ranker_batch* batch, void* ws, size_t ws_bytes);
/* mi_ranker_step_f32 that also says which launch forms it took.  Where the customer-side and the article-side twin of a step
 * share a kernel instantiation the executor issues them as ONE launch; otherwise, and always with an auxiliary stream, as two
 * single launches.  Both forms compute the same bits, so nothing but this report tells them apart.  `report` is zeroed at
 * entry and filled on the host before the call returns (the launch pass only: a declined call leaves it zero); null = plain
 * mi_ranker_step_f32.  One count per DECISION, not per kernel:
 *   merged[kind]: how often the one-launch form took the work;  single[kind]: how often the separate launches ran instead.
 *   EMBED               the two embedding lookups
 *   PREP_DROPOUT        the first encoder layer's two input dropouts: merged = inside the prep launch (p > 0, L > 1 only)
 *   DROPOUT             a later encoder layer's two input dropouts (forward)
 *   SPMM_FWD, SPMM_BWD  the two relations' aggregations of a layer (backward: layers above the first only)
 *   BN_FWD, BN_BWD      the two BatchNorms
 *   GATHER_CAT_DROPOUT  merged = the decoder's gather writes the dropped rows itself; single = the plain gather launch
 *   LINEAR1_BWD         merged = the last decoder layer's backward with its reduction in the same launch; single = two launches
 *   GATHER_CAT_BWD      the two sums of the gather's backward
 *   WGRAD               merged = launches of the transposed-product kernel (one for all layers when L <= 2, else one per
 *                       layer); single = layers whose weight gradients went through the grouped GEMM instead */
enum {
    MI_RANKER_LAUNCH_EMBED = 0, MI_RANKER_LAUNCH_PREP_DROPOUT = 1, MI_RANKER_LAUNCH_DROPOUT = 2, MI_RANKER_LAUNCH_SPMM_FWD = 3,
    MI_RANKER_LAUNCH_BN_FWD = 4, MI_RANKER_LAUNCH_GATHER_CAT_DROPOUT = 5, MI_RANKER_LAUNCH_LINEAR1_BWD = 6,
    MI_RANKER_LAUNCH_GATHER_CAT_BWD = 7, MI_RANKER_LAUNCH_BN_BWD = 8, MI_RANKER_LAUNCH_SPMM_BWD = 9, MI_RANKER_LAUNCH_WGRAD = 10,
    MI_RANKER_LAUNCH_KINDS = 11
};
typedef struct mi_ranker_launches {
    int32_t merged[MI_RANKER_LAUNCH_KINDS];
    int32_t single[MI_RANKER_LAUNCH_KINDS];
} mi_ranker_launches;
int    mi_ranker_step_report_f32(const mi_ranker_model* model, const mi_ranker_batch* batch, void* ws, size_t ws_bytes,
                                 mi_stream_t stream, mi_ranker_launches* report);
/* The update alone, for data-parallel callers: run mi_ranker_step_f32 with apply_adam = 0, all-reduce(sum) the gradient
 * buffers (params[i].g; the host side keeps them in ONE flat allocation so that is one collective), then this:
 * Adam (a9's arithmetic, model->lr/beta/eps/step) over model->params with every gradient multiplied by grad_scale
 * (1 / world size) first.  The gradient buffers are left as reduced (unscaled).  One launch. */
int    mi_ranker_adam_f32(const mi_ranker_model* model, float grad_scale, mi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * N3  candidate matcher: items bought by users who share an item with the query user.
 * replaces: UsersWithCommonItemsMatcher.get_matches at
 *           data/matching/users_with_common_purchases.py:14-26 (flatten of the co-purchasers'
 *           lists, t.cat of all their article lists, [:k]).
 * users_ptr/users_idx and articles_ptr/articles_idx: the adjacency lists IN LIST ORDER (the
 * reference's edges_*.pt / rev_edges_*.pt) as int32 CSR on device.  query_users int64[n] (null =
 * users 0..n-1).  out int32[n, k]: the first k entries of the concatenation, -1 padded;
 * out_count int32[n] (nullable): entries written.  One wavefront per query, stops at k.
 * ---------------------------------------------------------------------------------- */
int mi_match_common_items_i32(int64_t n_queries, const int64_t* query_users,
                              const int32_t* users_ptr, const int32_t* users_idx,
                              const int32_t* articles_ptr, const int32_t* articles_idx,
                              int32_t k, int32_t* out, int32_t* out_count, mi_stream_t stream);

/* N3  candidate matcher: items bought by the customers at the query user's location.
 * replaces: UsersSameLocationMatcher.get_matches at data/matching/fashion/users_same_location.py:15-25
 *           (t.cat of the article lists of customers_per_location[location_for_user[u]], [:k]).
 * location_of_user int32[num_users] (negative = unknown: no proposals); loc_ptr/loc_idx: customers per location in
 * list order; users_ptr/users_idx as above.  Output as mi_match_common_items_i32. */
int mi_match_same_location_i32(int64_t n_queries, const int64_t* query_users, const int32_t* location_of_user,
                               const int32_t* loc_ptr, const int32_t* loc_idx,
                               const int32_t* users_ptr, const int32_t* users_idx,
                               int32_t k, int32_t* out, int32_t* out_count, mi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * N3b  candidate matcher: scored item co-occurrence (item-to-item co-purchase similarity).
 * replaces: nothing.  The reference has no such matcher: its UsersWithCommonItemsMatcher keeps the
 *           first k entries of the user -> item -> user -> item walk and never counts how often an
 *           item is reached.  This is the scored form of that walk, in two stages.
 * Inputs of both stages: the adjacency lists IN LIST ORDER as int32 CSR on device, as
 * mi_match_common_items_i32 takes them; the two lists are transposes of one another and repeated
 * purchases are repeated entries of both.
 *
 * Stage 1, mi_cooc_items_topt: the item neighbour table.  d_i = length of article i's list;
 * c(i, j), i != j = number of walks i -> u -> j, one per position of u in i's list times every
 * position of j in u's list (= (A^T A)[i, j] with A[u, i] the multiplicity).  Score s(i, j) = c
 * (weighting MI_COOC_COUNT) or c / sqrt(d_i * d_j) in fp32 (MI_COOC_COSINE).  Row i of
 * nbr_id / nbr_count int32[n_items, T] and nbr_score float[n_items, T] holds the T best j with c > 0
 * by (s descending, j ascending), padded with id -1, count 0, score 0.  1 <= T <= 64.  Counts are
 * exact (integer LDS atomics) and every output is bit-identical from call to call; a count is
 * assumed to fit int32.  One workgroup per item row, heaviest rows first, the row's expansion
 * re-walked once per band of 36 864 item ids; the workspace holds the row order only.
 *
 * Stage 2, mi_match_cooc_i32: r(u, j) = sum over the list positions p taken of nbr_score[L_u[p], t]
 * over every t with nbr_id[L_u[p], t] == j, summed in (p, t) order.  Positions taken: all of L_u,
 * or the last n_recent (n_recent <= 0 = all; list order is transaction order).  exclude_seen != 0
 * drops every item anywhere in the user's whole list.  out int32[n, k]: the k best j with r > 0 by
 * (r descending, j ascending), -1 padded; out_score float[n, k] (nullable): their r, 0 padded;
 * out_count int32[n] (nullable): entries written.  query_users int64[n] (null = users 0..n-1; any
 * order, repeats allowed).  max_list_len: an upper bound of the longest purchase list among the
 * queried users; it sizes the workspace slabs in which users whose |L_u| * T terms do not fit LDS
 * are sorted (exactly: nothing is truncated).  A queried user whose list is longer than
 * max_list_len gets no candidates and out_count -1.
 *
 * The size queries run without a GPU and return 0 for arguments the calls refuse.  Null pointers,
 * T outside 1..64, k <= 0, an unknown weighting and nnz >= 2^31 return MI_ERR_BAD_ARG before any
 * launch; a short workspace returns MI_ERR_WORKSPACE.
 * ---------------------------------------------------------------------------------- */
#define MI_COOC_COUNT  0
#define MI_COOC_COSINE 1
size_t mi_cooc_items_workspace_bytes(int64_t n_items, int64_t nnz, int32_t T);
int    mi_cooc_items_topt(int64_t n_users, int64_t n_items, int64_t nnz,
                          const int32_t* users_ptr, const int32_t* users_idx,
                          const int32_t* articles_ptr, const int32_t* articles_idx,
                          int32_t T, int32_t weighting,
                          int32_t* nbr_id, int32_t* nbr_count, float* nbr_score,
                          void* ws, size_t ws_bytes, mi_stream_t stream);
size_t mi_match_cooc_workspace_bytes(int64_t n_queries, int64_t max_list_len, int32_t T);
int    mi_match_cooc_i32(int64_t n_queries, const int64_t* query_users,
                         const int32_t* users_ptr, const int32_t* users_idx, int64_t max_list_len,
                         int32_t T, const int32_t* nbr_id, const float* nbr_score,
                         int32_t k, int32_t n_recent, int32_t exclude_seen,
                         int32_t* out, float* out_score, int32_t* out_count,
                         void* ws, size_t ws_bytes, mi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * N3c random-walk matcher: Pixie-style candidates for a user, by walking from the items they hold
 *      (additive to ABI 14; csrc/walk_match.hip).
 * replaces: nothing.  The reference's two walks keep the first k entries of an unscored expansion;
 *           mi_pinsage_neighbors / mi_pinsage_hard_negatives walk from ONE item.  This walks from a
 *           user's recent items, counts where the walks end and ranks by the counts.  It needs no
 *           training and no table: an edge counts the moment it is in the two CSRs.
 * Inputs: iu_ptr / iu_idx (item -> users) and ui_ptr / ui_idx (user -> items) as int32 CSR on device,
 * transposes of one another, user rows in transaction order.  ui_sorted: a copy of ui_idx with every
 * row sorted by item id (read only with exclude_seen; null otherwise).
 *
 * The rule for query user u at (seed, step), restated in numpy by tests/random_walk_matcher_emulation.py:
 *   slots     the history rule of the recent-items recommender (N5 below): the last min(len, 64)
 *             entries of row u, most recent first, an entry dropped when a more recent position holds
 *             its item; the first n_recent survivors are slots 0 .. R - 1, 1 <= n_recent <=
 *             MI_RECENT_MAX_SLOTS.  An empty row (or an id outside [0, n_users)) has R = 0 and gets no
 *             proposal: ids -1, scores 0, count 0.  That is not an error.
 *   walks     num_walks walks; walk w starts at the item of slot w % R and makes at most walk_length
 *             item -> user -> item traversals under mi_pinsage_neighbors' law.  Traversal t of walk w
 *             draws x = Philox(purpose 17, a = w * walk_length + t, b = 0, c = u, seed, step) in the
 *             PinSAGE counter layout.  Before every traversal but the first the walk ends if
 *             x.c[2] < (uint32)(restart_prob * 2^32); otherwise the hop takes user
 *             iu[item][x.c[0] % len] and item ui[user][x.c[1] % len]; a walk that meets an item
 *             without users ends.  The draws are keyed on the user id, not on the query position: a
 *             user's answer does not depend on who else is queried, or in which order.
 *   counts    c[r][i] = number of traversal ends at item i among the walks of slot r.
 *   eligible  exclude_seen != 0 drops every item of u's WHOLE row (not only the slots); 0 drops nothing.
 *   score     MI_WALK_BOOST_SUM: s(i) = sum_r c[r][i], an integer <= 4096, exact in float.
 *             MI_WALK_BOOST_MULTI_HIT (Pixie's booster): s(i) = (sum_r sqrt(c[r][i]))^2 in float over
 *             the slots with c > 0 in ascending r: every root the correctly rounded float root, every
 *             addition (from 0) and the final multiply rounded once, no contraction.
 *   answer    the k best eligible items with s > 0 by (s descending, id ascending).  out_ids
 *             int32[n, k], -1 padded; out_scores float[n, k] (nullable), 0 padded; out_count int32[n]
 *             (nullable): the distinct eligible items visited, before the cut to k.
 * One workgroup per query; visits are sorted in LDS: num_walks * walk_length <=
 * MI_WALK_MATCH_MAX_VISITS, beyond that MI_ERR_UNSUPPORTED.  n_items < 2^31 - 1 (MI_ERR_TOO_LARGE).
 * MI_ERR_BAD_ARG: num_walks, walk_length or k <= 0, restart_prob outside [0, 1), n_recent outside
 * 1 .. MI_RECENT_MAX_SLOTS, an unknown boost, a negative count, a null or misaligned pointer.  All of
 * these are returned before anything is enqueued; zero queries return 0 with nothing enqueued.
 * query_users int64[n] (null = users 0 .. n - 1; any order, repeats allowed).  No float atomics, no
 * global scratch, one writer per output: two calls give equal bits.
 * ---------------------------------------------------------------------------------- */
#define MI_WALK_BOOST_SUM        0
#define MI_WALK_BOOST_MULTI_HIT  1
#define MI_WALK_MATCH_MAX_VISITS 4096
int    mi_match_random_walks_i32(int64_t n_queries, const int64_t* query_users, int64_t n_users, int64_t n_items,
                                 const int32_t* iu_ptr, const int32_t* iu_idx,
                                 const int32_t* ui_ptr, const int32_t* ui_idx, const int32_t* ui_sorted,
                                 int32_t k, int32_t num_walks, int32_t walk_length, double restart_prob,
                                 int32_t n_recent, int32_t boost, int32_t exclude_seen,
                                 uint64_t seed, uint64_t step,
                                 int32_t* out_ids, float* out_scores, int32_t* out_count, mi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * N1  on-device N-hop subgraph sampler for the ranker.
 * replaces: GraphDataset.__getitem__ + helpers (data/dataset.py:39-309, train mode) for a whole
 *           batch of seed users, and the PyG collate of the resulting HeteroData items
 *           (data/data_loader.py:48): sampled positive label edges (with
 *           replacement), negatives (fast path / exact path), the seed user's own edges, the
 *           N-hop neighbourhood with the fan-out cap on both frontiers, sorted-unique relabelling.
 * users_ptr/users_idx: CSR user -> article ids IN LIST ORDER (edges_*.pt); articles_ptr/idx:
 * CSR article -> user ids (rev_edges_*.pt); all int32, device.  id_max = max article id of the
 * graph, num_edges its edge count (the fast-path test E / n_neg > 100).  max_pos / max_neg:
 * capacity per sample of the label lists, >= max(2, floor(max_degree*ratio)) and
 * >= max(k-1, int(neg_ratio*max_pos)).
 * Two calls per batch because the output sizes are data dependent:
 *   mi_sampler_count  runs the walk, SYNCHRONISES, returns totals_host[4] = {user nodes,
 *                     article nodes, message-passing edges, label edges} of the collated batch;
 *   mi_sampler_count_async  the same without the wait: the four totals land in caller-owned host
 *                     memory (pin it) when `stream` reaches that point — the caller waits on an event
 *                     of its own, so a batch can be sampled on a side stream while the previous one trains;
 *   mi_sampler_emit   writes user_ids int64[tot0], article_ids int64[tot1] (global ids, sorted
 *                     within each sample), edge_index int64[2, tot2], edge_label_index
 *                     int64[2, tot3] (batch-local ids), edge_label int64[tot3],
 *                     user_ptr / article_ptr int64[batch+1] (node offsets per sample).
 *   mi_sampler_emit_csr  (optional, after mi_sampler_count*, same ws) writes the SAME message-passing edges as the
 *                     two CSRs mi_coo_to_csr_i32 would build from edge_index — customers x articles
 *                     (customer_rowptr int32[tot0+1], customer_col int32[tot2]) and articles x customers
 *                     (article_rowptr int32[tot1+1], article_col int32[tot2]), both sorted by (row, column),
 *                     batch-local ids — so the encoder needs no sort per batch (model/layers.py BipartiteGraph;
 *                     replaces the SparseTensor construction inside PyG's SAGEConv propagate).  article_cursor:
 *                     int32[tot1] scratch.  MI_ERR_UNSUPPORTED when n_hops*num_neighbors > 512.
 * Frontier: when the queued articles' user lists total more than reject_min_entries, the
 * uniform num_neighbors-subset of their distinct unexplored users is drawn by rejection (position of
 * the concatenated lists, acceptance 1/multiplicity) instead of materialising the set — hub
 * articles carry 10^5..10^6 users; the bound guarantees >= num_neighbors candidates exist.
 * Randomness: Philox4x32-10 keyed on (seed, step); bit-exact mirror in oracle/sampler_ref.py.
 * ---------------------------------------------------------------------------------- */
typedef struct mi_sampler_desc {
    int32_t batch, n_hops, num_neighbors, k;
    int32_t randomization, max_pos, max_neg, reserved;
    int64_t num_users, num_articles, num_edges, id_max;
    const int32_t* users_ptr;    const int32_t* users_idx;
    const int32_t* articles_ptr; const int32_t* articles_idx;
    double positive_edges_ratio, negative_edges_ratio;
    int64_t reject_min_entries; /* 0 = default 4*n*(n*(hops+1)+1); must be >= n*(n*(hops+1)+1) */
    /* evaluation mode (data/dataset.py:94-105, train=False): when cand_ptr is non-null the label-0 edges of seed
     * user u are not sampled but the ids that occur exactly once in cat(unique(candidates of u), items of u) —
     * candidates that are not purchases plus, as the reference writes it, purchases no matcher proposed — in
     * ascending order.  cand_ptr int32[num_users + 1] / cand_idx int32[]: the matchers' proposals per user
     * (duplicates allowed, any order).  max_neg >= max_u(candidates of u + items of u). */
    const int32_t* cand_ptr;     const int32_t* cand_idx;
} mi_sampler_desc;

size_t mi_sampler_workspace_bytes(const mi_sampler_desc* d);
int    mi_sampler_count(const mi_sampler_desc* d, const int64_t* seed_users, uint64_t seed, uint64_t step,
                        void* ws, size_t ws_bytes, int64_t* totals_host, mi_stream_t stream);
int    mi_sampler_count_async(const mi_sampler_desc* d, const int64_t* seed_users, uint64_t seed, uint64_t step,
                              void* ws, size_t ws_bytes, int32_t* totals_pinned, mi_stream_t stream);
int    mi_sampler_emit(const mi_sampler_desc* d, const int64_t* seed_users, void* ws, size_t ws_bytes,
                       const int64_t* totals_host, int64_t* user_ids, int64_t* article_ids,
                       int64_t* edge_index, int64_t* edge_label_index, int64_t* edge_label,
                       int64_t* user_ptr, int64_t* article_ptr, mi_stream_t stream);
/* mi_sampler_emit with edge_index / edge_label_index written as [3, n] when three_rows != 0: row 2 repeats row 0, so rows 0..1
 * are the `buys` relation's index and rows 1..2 the reversed relation's (`rev_buys`: data/dataset.py builds it with flip(0)) —
 * two views of one buffer instead of two flip launches per batch (round 4). */
int    mi_sampler_emit3(const mi_sampler_desc* d, const int64_t* seed_users, void* ws, size_t ws_bytes,
                        const int64_t* totals_host, int64_t* user_ids, int64_t* article_ids,
                        int64_t* edge_index, int64_t* edge_label_index, int64_t* edge_label,
                        int64_t* user_ptr, int64_t* article_ptr, int32_t three_rows, mi_stream_t stream);
int    mi_sampler_emit_csr(const mi_sampler_desc* d, void* ws, size_t ws_bytes, const int64_t* totals_host,
                           int32_t* customer_rowptr, int32_t* customer_col, int32_t* article_rowptr,
                           int32_t* article_col, int32_t* article_cursor, mi_stream_t stream);

/* N1b  attribute node types of the ranker's batches (Config.other_edge_types; the reference's default dataset puts
 *      them into every batch: data/dataset_neo.py:67-91,140-168).  A relation (article, name, T) is a CSR over the
 *      articles: rel_ptr int32[num_articles + 1], rel_idx int32[nnz], every row STRICTLY ascending, ids in
 *      [0, n_targets) (checked by the caller: the kernels index bitmaps with them), 1 <= n_targets <= 2^31 - 1.  Up to
 *      MI_SAMPLER_MAX_RELATIONS relations per call.  The rule, per sample s of the collated batch, whose articles are
 *      a_0 < ... < a_{m-1} at batch-local indices article_ptr[s] + j (all of them: label articles too, train or
 *      evaluation mode):
 *        T nodes of s   the sorted distinct ids of the union of rel[a_j]; t_ptr[s] = their number in samples < s;
 *                       t_ids[t_ptr[s] + r] = the r-th of them (global id);
 *        edges of s     for j ascending and, within j, e in rel[a_j] ascending:
 *                       (article_ptr[s] + j, t_ptr[s] + rank_s(e)); the samples' edges follow one another in sample order.
 *      Attribute nodes are never expanded into further articles, and the walk's draws do not depend on the relations.
 *   mi_sampler_count_relations_async   after mi_sampler_count / mi_sampler_count_async of the same batch, same stream,
 *                       same ws (read only): builds the per-sample T sets in rel_ws (which it clears itself: a batch
 *                       that was counted and never emitted leaves nothing behind) and copies
 *                       totals_pinned[2 r + {0, 1}] = {T nodes, edges} of relation r to caller-owned pinned host
 *                       memory when the stream gets there (-1: the count does not fit int32) — behind the same event
 *                       as the walk's four totals, no host wait of its own.
 *   mi_sampler_emit_relations   same ws / rel_ws, untouched in between; totals_host = the walk's four totals,
 *                       rel_totals_host[2 n_rel] the ones above.  Writes per relation, with nt / ne its totals and
 *                       na = totals_host[1]:
 *                         t_ids int64[nt], t_ptr int64[batch + 1];
 *                         edge3 int64[3, ne]: row 0 the article, row 1 the T node (batch-local), row 2 = row 0 again, so
 *                           rows 0..1 are the relation's edge_index and rows 1..2 the reversed relation's (as
 *                           mi_sampler_emit3 does for buys / rev_buys);
 *                         articles x T: article_rowptr int32[na + 1], article_col int32[ne];
 *                         T x articles: t_rowptr int32[nt + 1], t_col int32[ne]; both sorted by (row, column) — what
 *                           mi_coo_to_csr_i32 would build from edge3.  t_cursor: int32[nt] scratch.
 *                       The transposed rows are filled in edge order, which is ascending article order: no sort, and no
 *                       atomic whose order could reach the output.  Pointers may be null where the size is 0.
 * Everything is validated before anything is enqueued (pointers, alignment, n_rel, n_targets, workspace sizes). */
#define MI_SAMPLER_MAX_RELATIONS 4
typedef struct mi_sampler_relation {
    const int32_t* rel_ptr;
    const int32_t* rel_idx;
    int64_t n_targets;
} mi_sampler_relation;

typedef struct mi_sampler_relation_out {
    int64_t* t_ids; int64_t* t_ptr; int64_t* edge3;
    int32_t* article_rowptr; int32_t* article_col;
    int32_t* t_rowptr; int32_t* t_col; int32_t* t_cursor;
} mi_sampler_relation_out;

size_t mi_sampler_relations_workspace_bytes(const mi_sampler_desc* d, const mi_sampler_relation* rels, int32_t n_rel);
int    mi_sampler_count_relations_async(const mi_sampler_desc* d, const mi_sampler_relation* rels, int32_t n_rel,
                                        void* ws, size_t ws_bytes, void* rel_ws, size_t rel_ws_bytes,
                                        int32_t* totals_pinned, mi_stream_t stream);
int    mi_sampler_emit_relations(const mi_sampler_desc* d, const mi_sampler_relation* rels, int32_t n_rel,
                                 void* ws, size_t ws_bytes, const int64_t* totals_host, void* rel_ws,
                                 size_t rel_ws_bytes, const int64_t* rel_totals_host,
                                 const mi_sampler_relation_out* outs, mi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * N5  PinSAGE samplers (reference: pinsage/sampler.py:16-106 over DGL's random_walk and
 *     PinSAGESampler; DGL is absent and the reference's pinsage/ cannot import — SURVEY F11 — so the
 *     semantics are restated in oracle/pinsage_ref.py, which mirrors these kernels bit for bit).
 * iu_*: CSR item -> users; ui_*: CSR user -> items (int32, device).
 * mi_pinsage_item_pairs: heads uniform over items; tails[b] = end of one item->user->item walk from
 *   heads[b] (uniform neighbour per step), -1 when the walk dies; neg_tails uniform.  int64[batch] each.
 * mi_pinsage_neighbors: per seed, num_walks walks of walk_length traversals with termination
 *   probability restart_prob before every traversal but the first; the items reached at the end of
 *   each traversal are counted and the num_neighbors most visited (count desc, id asc) returned:
 *   neighbors int64[n_seeds, T] (-1 padded), weights int64[n_seeds, T] (visit counts).
 * ---------------------------------------------------------------------------------- */
int    mi_pinsage_item_pairs(int64_t batch, int64_t n_items,
                             const int32_t* iu_ptr, const int32_t* iu_idx,
                             const int32_t* ui_ptr, const int32_t* ui_idx,
                             uint64_t seed, uint64_t step,
                             int64_t* heads, int64_t* tails, int64_t* neg_tails, mi_stream_t stream);
size_t mi_pinsage_neighbors_workspace_bytes(int64_t n_seeds, int32_t walk_length, int32_t num_walks);
int    mi_pinsage_neighbors(int64_t n_seeds, const int64_t* seeds,
                            const int32_t* iu_ptr, const int32_t* iu_idx,
                            const int32_t* ui_ptr, const int32_t* ui_idx,
                            int32_t walk_length, double restart_prob, int32_t num_walks,
                            int32_t num_neighbors, int32_t layer, uint64_t seed, uint64_t step,
                            int64_t* neighbors, int64_t* weights,
                            void* ws, size_t ws_bytes, mi_stream_t stream);

/* N5, whole batch on the device (round 3): item pairs -> seeds -> per layer (neighbours -> block), six launches for the
 * reference's two layers, no host read-back inside.  replaces: sample_from_item_pairs + sample_blocks at
 * pinsage/sampler.py:73-106 (dgl.to_block numbering: destination nodes first, new sources ascending; frontier edges
 * that repeat a label pair removed) AND the two sorts per block the model needed for its weighted-mean aggregation
 * (pinsage/layers.py:150-160): every block comes with its CSR by destination and by source, values
 * w / max(sum of the destination's w, 1).
 * Buffers are sized for the upper bounds n_max(0) = 3 * batch, n_max(l + 1) = n_max(l) * (1 + num_neighbors); the actual
 * counts land in counts: [0] surviving pairs, [1] seeds, [2 + 2l] nodes of block l, [3 + 2l] edges of block l (block 0 =
 * the one built FIRST, around the seeds; the model consumes them in reverse).  MI_ERR_UNSUPPORTED when batch > 1024 or a
 * layer's n_max * num_neighbors exceeds 16384 (the caller then builds the blocks with its own index ops). */
#define MI_PINSAGE_MAX_LAYERS 4
typedef struct mi_pinsage_batch_desc {
    int64_t batch, n_items;
    const int32_t *iu_ptr, *iu_idx, *ui_ptr, *ui_idx;
    int32_t walk_length, num_walks, num_neighbors, num_layers;
    double  restart_prob;
    int32_t* pos_scratch;          /* device int32[n_items], all -1 on entry and on return */
} mi_pinsage_batch_desc;
typedef struct mi_pinsage_block_out {
    int64_t *src_ids, *edge_src, *edge_dst;   /* [n_max*(1+T)], [n_max*T], [n_max*T] */
    float*   weights;                          /* [n_max*T] visit counts */
    int32_t *dst_rowptr, *dst_col; float* dst_val;   /* [n_max+1], [n_max*T], [n_max*T] */
    int32_t *src_rowptr, *src_col; float* src_val;   /* [n_max*(1+T)+1], [n_max*T], [n_max*T] */
} mi_pinsage_block_out;
typedef struct mi_pinsage_batch_out {
    int64_t *seeds, *pos_u, *pos_v, *neg_v;   /* [3*batch], [batch] x 3: positions of head / tail / negative in seeds */
    int32_t* counts;                          /* [2 + 2*num_layers] */
    mi_pinsage_block_out blocks[MI_PINSAGE_MAX_LAYERS];
} mi_pinsage_batch_out;
size_t mi_pinsage_batch_workspace_bytes(int64_t batch, int32_t walk_length, int32_t num_walks, int32_t num_neighbors,
                                        int32_t num_layers);
int    mi_pinsage_sample_batch(const mi_pinsage_batch_desc* desc, uint64_t seed, uint64_t step,
                               const mi_pinsage_batch_out* out, void* ws, size_t ws_bytes, mi_stream_t stream);

/* N5, hard negatives from random-walk ranks (PinSAGE paper, section 3.3; neither the reference nor DGL's example has them):
 * items related to the head but ranked below its true neighbours by visit count replace a share of the uniform negatives.
 * The rule, for pair b of the batch at (seed, step), after mi_pinsage_item_pairs wrote heads[b] = h, tails[b] = tl and the
 * uniform neg_tails[b] (Philox counters laid out as for the other PinSAGE draws: (a, b, c, purpose | step << 8)):
 *   dead pairs   tl == -1: the pair is left alone.
 *   selection    pk = Philox(purpose 15, a = b, 0, 0, seed, step); the pair is hard iff share >= 1 or
 *                pk.c[0] < (uint32)(share * 2^32); otherwise neg_tails[b] stays uniform.
 *   walks        num_walks walks from h of at most walk_length item -> user -> item traversals under mi_pinsage_neighbors'
 *                law: before every traversal but the first the walk ends if w.c[2] < (uint32)(restart_prob * 2^32); the hop
 *                takes w.c[0] (user) and w.c[1] (item); a walk that meets an item without users ends.  Draws:
 *                w = Philox(purpose 16, a = walk * walk_length + traversal, 0, h, seed, step) — keyed on the head item, so
 *                two pairs with one head share their walks and differ only in pk.
 *   counting     every item reached at the end of a traversal is counted; then h and tl are removed from the counts.
 *   ranking      the remaining m distinct items are ranked by (count desc, id asc); end = min(rank_hi, m); if end <= rank_lo
 *                the uniform negative stays, otherwise neg_tails[b] = the item at rank rank_lo + pk.c[1] % (end - rank_lo).
 * One workgroup per pair, visits sorted in LDS: num_walks * walk_length <= 4096, beyond that MI_ERR_UNSUPPORTED.  Argument
 * errors (num_walks, walk_length <= 0; restart_prob outside [0, 1); share outside [0, 1]; rank_lo < 0; rank_hi <= rank_lo)
 * and the limit are reported before anything is enqueued.
 * mi_pinsage_hard_negatives: neg_tails holds the uniform negatives on entry; rank_out (nullable, int32[batch]) receives for
 *   every pair the rank taken, or -1 where the uniform negative stayed or the pair is dead.
 * mi_pinsage_sample_batch_hard: mi_pinsage_sample_batch with that launch between the item pairs and the seeds, so that the
 *   seeds, the positions and the banned label-pair keys come from the final negatives; hn == NULL or share == 0 enqueues
 *   exactly mi_pinsage_sample_batch's launches.  mi_pinsage_batch_workspace_bytes sizes the workspace. */
typedef struct mi_pinsage_hard_neg { int32_t num_walks, walk_length, rank_lo, rank_hi; double restart_prob, share; } mi_pinsage_hard_neg;
int64_t mi_pinsage_hard_sizeof(void);                       /* binding self-check */
int    mi_pinsage_hard_negatives(int64_t batch, int64_t n_items,
                                 const int32_t* iu_ptr, const int32_t* iu_idx,
                                 const int32_t* ui_ptr, const int32_t* ui_idx,
                                 const mi_pinsage_hard_neg* hn, uint64_t seed, uint64_t step,
                                 const int64_t* heads, const int64_t* tails, int64_t* neg_tails,
                                 int32_t* rank_out, mi_stream_t stream);
int    mi_pinsage_sample_batch_hard(const mi_pinsage_batch_desc* desc, const mi_pinsage_hard_neg* hn,
                                    uint64_t seed, uint64_t step, const mi_pinsage_batch_out* out,
                                    void* ws, size_t ws_bytes, mi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * N5  one PinSAGE training iteration as ONE call (round 3).
 * replaces: the loop body of pinsage/model.py:118-131 (train) on PinSAGEModel (pinsage/model.py:16-34): LinearProjector
 *           over the item-id feature (an embedding row per node), SAGENet of WeightedSAGEConv layers
 *           (pinsage/layers.py:121-156: n = relu(Q dropout(h_src)), weighted mean over the sampled neighbours,
 *           z = relu(W dropout([agg, h_dst])), row L2-normalisation), h_dst + SAGENet output, ItemToItemScorer
 *           (pinsage/layers.py:181-203: dot + both endpoints' bias), hinge (neg - pos + 1).clamp(min = 0).mean(),
 *           backward, torch.optim.Adam step.  Issued op by op through autograd the iteration is ~200 launches of a few
 *           microseconds (1.8 ms at the reference's 32 pairs per batch); here ~40.
 * The batch is one built by mi_pinsage_sample_batch (blocks in MODEL order: input layer first; destination nodes are the
 * first rows of every block's src_ids, so the seeds are the first n_seeds rows of block 0's).  Dropout: Philox4x32-10
 * masks keyed on (seed, step, site), regenerated in the backward.  Gradients: the embedding table's and the scorer
 * bias's gradient buffers are DENSE and must be all zero on entry; the rows of this batch are written, Adam runs over
 * the whole tables (torch.optim.Adam's dense semantics: every moment decays every step) and the rows are zeroed again
 * — unless apply_adam = 0, which stops after the gradients and leaves them in place (the caller zeroes them).
 * hidden % 4 == 0, hidden <= 128.  Everything is deterministic (no float atomics).
 * ---------------------------------------------------------------------------------- */
#define MI_PINSAGE_MAX_PARAMS 24
typedef struct mi_pinsage_conv {
    const float *q_w, *q_b, *w_w, *w_b;        /* Q [hidden, hidden] + [hidden]; W [hidden, 2 hidden] + [hidden] */
    float *g_q_w, *g_q_b, *g_w_w, *g_w_b;      /* gradients, same shapes */
} mi_pinsage_conv;
typedef struct mi_pinsage_model {
    int32_t n_layers, hidden;
    int64_t n_items;
    float *proj, *g_proj, *m_proj, *v_proj;    /* [n_items + 1, hidden]: table, dense gradient (zero on entry), Adam moments */
    const float* bias; float* g_bias;          /* [n_items] scorer bias and its dense gradient (zero on entry) */
    mi_pinsage_conv conv[MI_PINSAGE_MAX_LAYERS];
    mi_ranker_param params[MI_PINSAGE_MAX_PARAMS];   /* every parameter EXCEPT proj (the scorer bias included): multi-tensor Adam */
    int32_t n_params, apply_adam;
    float   p_dropout; int32_t reserved;
    double  lr, beta1, beta2, eps;
    int64_t step;                               /* Adam step of THIS iteration, counts from 1 */
    const float* ones4; int64_t n_ones;         /* [n_ones, 4] ones, n_ones >= the largest block's n_src */
} mi_pinsage_model;
typedef struct mi_pinsage_step_block {
    int64_t n_src, n_dst, nnz;
    const int64_t* src_ids;                                      /* [n_src] global item ids, destination nodes first */
    const int32_t *dst_rowptr, *dst_col; const float* dst_val;   /* CSR by destination [n_dst x n_src], w / max(sum w, 1) */
    const int32_t *src_rowptr, *src_col; const float* src_val;   /* the same entries by source [n_src x n_dst] */
} mi_pinsage_step_block;
typedef struct mi_pinsage_step_batch {
    int32_t n_blocks, reserved;
    mi_pinsage_step_block blocks[MI_PINSAGE_MAX_LAYERS];         /* model order */
    int64_t n_seeds, n_pairs;
    const int64_t *seeds, *pos_u, *pos_v, *neg_v;                /* [n_seeds] ids; [n_pairs] positions in seeds */
    uint64_t seed, step;                                         /* dropout stream */
    float*   loss;                                               /* device float[1] */
    /* data-parallel callers (both or neither; requires model->apply_adam = 0): the projector / bias gradients of THIS batch
     * are written compactly — rows_out [blocks[0].n_src, hidden] (row r belongs to item blocks[0].src_ids[r]), bias_out
     * [n_seeds] (entry s belongs to item seeds[s]) — instead of into the dense buffers, which are not touched. */
    float*   rows_out;
    float*   bias_out;
} mi_pinsage_step_batch;
/* One list of compact gradient rows (a rank's contribution), as written by mi_pinsage_step_f32 through rows_out / bias_out. */
typedef struct mi_pinsage_grad_list {
    int64_t n_rows, n_seeds;
    const int64_t* ids;        /* [n_rows] distinct item ids; the first n_seeds are the seeds */
    const float*   rows;       /* [n_rows, hidden] */
    const float*   bias;       /* [n_seeds] */
} mi_pinsage_grad_list;
int64_t mi_pinsage_step_sizeof(int32_t which);  /* sizeof of: 0 model, 1 batch, 2 conv, 3 block, 4 grad list (binding self-check) */
size_t mi_pinsage_step_workspace_bytes(const mi_pinsage_model* model, const mi_pinsage_step_batch* batch);
int    mi_pinsage_step_f32(const mi_pinsage_model* model, const mi_pinsage_step_batch* batch, void* ws, size_t ws_bytes,
                           mi_stream_t stream);
/* The validation pass of mi_pinsage_step_f32 alone (see mi_ranker_step_check): nothing enqueued, no device memory read. */
int    mi_pinsage_step_check(const mi_pinsage_model* model, const mi_pinsage_step_batch* batch, void* ws, size_t ws_bytes);
/* The update of a data-parallel iteration: the lists of every rank (exchanged by the caller: an all-gather of a few hundred
 * KB instead of an all-reduce of the dense 27 MB table gradient), in rank order, are added into the zero-kept dense
 * buffers — projector rows times grad_scale (1 / world), bias entries as they are; lists are applied one after the other,
 * ids within a list are distinct: one writer per entry at any time, the sum does not depend on scheduling — then Adam over
 * model->params with every gradient times grad_scale (the caller has all-reduced(sum) those dense gradients), the dense
 * Adam over the projector table, and the touched rows / entries are cleared again.  n_lists <= 64. */
int    mi_pinsage_apply_f32(const mi_pinsage_model* model, const mi_pinsage_grad_list* lists, int32_t n_lists, float grad_scale,
                            mi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * N5  evaluation: the representation of EVERY item in one call (round 5).
 * replaces: the evaluation half of pinsage/model.py:120-134 — collate_test's sample_blocks over batches of item ids
 *           (pinsage/sampler.py:181-185) and model.get_repr per batch, in eval mode (no dropout).
 * For one (seed, step) an item's top-T neighbours at a sampler layer do not depend on the batch it is in (the walk draws
 * are keyed on the start item; eval blocks carry no label pairs), so the batched get_repr equals a layer-by-layer pass
 * over the catalogue: per model layer m, the neighbours of every item at sampler layer n_layers - 1 - m (the draws of
 * mi_pinsage_neighbors over seeds 0 .. n_items - 1), n = relu(Q h + b_Q) over all items, then one fused kernel per item:
 * weighted mean of its neighbours' n rows (w / max(sum w, 1), ascending j), W [mean, h] + b_W, relu, L2 normalisation
 * (norm 0: divided by 1); out = proj + h of the last layer.  Equal to the batched path to rounding (the order of at most
 * T terms of the mean), not bitwise; deterministic, no atomics, nothing waited on by the host.
 * Reads of the model descriptor: n_layers, hidden, n_items, proj ([n_items + 1, hidden]; rows 0 .. n_items - 1 used) and
 * conv[l].q_w / q_b / w_w / w_b; nothing else.  out: [n_items, hidden] fp32.  proj, out and the biases 16-byte aligned.
 * MI_ERR_UNSUPPORTED (nothing enqueued) unless hidden % 4 == 0, hidden <= 128, 1 <= n_layers <= MI_PINSAGE_MAX_LAYERS,
 * num_neighbors <= 16 and the walks of one seed fit mi_pinsage_neighbors' block.
 * ---------------------------------------------------------------------------------- */
size_t mi_pinsage_embed_items_workspace_bytes(int64_t n_items, int32_t hidden, int32_t num_neighbors);
int    mi_pinsage_embed_items_f32(const mi_pinsage_model* model, const int32_t* iu_ptr, const int32_t* iu_idx,
                                  const int32_t* ui_ptr, const int32_t* ui_idx, int32_t walk_length, double restart_prob,
                                  int32_t num_walks, int32_t num_neighbors, uint64_t seed, uint64_t step, float* out,
                                  void* ws, size_t ws_bytes, mi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * N5  PinSAGE item feature projector (ABI 14).
 * replaces: LinearProjector (pinsage/layers.py:14-46, 90-118): every node feature column is projected to `hidden` and
 *           the results are summed — an embedding table per integer column, a Linear over the float columns, the item
 *           id being one more integer column.  With it an item that has no interactions still gets a representation.
 * Forward, for output row r (item i = ids ? ids[r] : r), ONE f32 addition chain in this order:
 *     id_table[i]  (if id_table)  +  tables[0][x[i, 0]]  + ... +  tables[n_cols - 1][x[i, n_cols - 1]]
 *     +  (dense[i, :] @ w^T + b)   (if n_dense > 0; the product is the k-ascending fma chain of mi_gemm_f32)
 * The codes x[i, c] index tables[c] UNCHECKED: the caller guarantees 0 <= x[i, c] < table_rows[c] (and ids < n_items).
 * Backward, given g = dL/d out [n, hidden]: every table row (id table included) that some r < n looks up is WRITTEN with
 * the sum of those g[r] (rows nobody looks up are not touched: the caller keeps the buffers zero, as the executor does
 * for g_proj); g_w = sum_r g[r]^T dense[i_r], g_b = sum_r g[r] are written whole.  The (column, code) references are
 * radix-sorted (stable: ascending r within a code), summed in 64-reference chunks with several row loads in flight and
 * the chunk partials of a run are combined in chunk order; g_b is a fixed-order column sum; g_w a trans_a product with
 * the launcher's split-K rule.  No float atomics: both calls give the same bits on every run.
 * hidden % 4 == 0, 4 <= hidden <= 128, n_cols <= 16 (MI_ERR_UNSUPPORTED otherwise); at least one of id_table, n_cols,
 * n_dense; tables, out, g and the gradient buffers 16-byte aligned with ldo / ldg % 4 == 0.  Everything is validated before
 * anything is enqueued.
 * ---------------------------------------------------------------------------------- */
#define MI_PROJECTOR_MAX_COLS 16
typedef struct mi_item_projector {
    int32_t hidden, n_cols;
    int64_t n_items;
    const int64_t* x;                               /* [n_items, n_cols] codes */
    const float*   tables[MI_PROJECTOR_MAX_COLS];   /* tables[c]: [table_rows[c], hidden] */
    int64_t        table_rows[MI_PROJECTOR_MAX_COLS];
    const float*   id_table;                        /* nullable; [>= n_items, hidden] */
    int64_t        n_dense;
    const float*   dense; int64_t ld_dense;         /* [n_items, n_dense], leading dimension in floats */
    const float*   w;                               /* [hidden, n_dense] */
    const float*   b;                               /* [hidden] */
} mi_item_projector;
typedef struct mi_item_projector_grads {           /* each with the shape of its parameter */
    float* g_tables[MI_PROJECTOR_MAX_COLS];
    float* g_id_table;
    float* g_w;
    float* g_b;
} mi_item_projector_grads;
int64_t mi_pinsage_project_sizeof(int32_t which);   /* sizeof of: 0 projector, 1 grads (binding self-check); else -1 */
size_t mi_pinsage_project_workspace_bytes(const mi_item_projector* p, int64_t n);
int    mi_pinsage_project_f32(const mi_item_projector* p, int64_t n, const int64_t* ids /* null = 0 .. n-1 */, float* out,
                              int64_t ldo, void* ws, size_t ws_bytes, mi_stream_t stream);
size_t mi_pinsage_project_bwd_workspace_bytes(const mi_item_projector* p, int64_t n);
int    mi_pinsage_project_bwd_f32(const mi_item_projector* p, const mi_item_projector_grads* grads, int64_t n,
                                  const int64_t* ids, const float* g, int64_t ldg, void* ws, size_t ws_bytes,
                                  mi_stream_t stream);
/* Zeroes again the table rows (id table included) that mi_pinsage_project_bwd_f32 wrote for the same (n, ids): how a caller
 * keeps the dense table gradients all-zero between iterations without clearing whole tables.  g_w / g_b are not touched. */
int    mi_pinsage_project_clear_f32(const mi_item_projector* p, const mi_item_projector_grads* grads, int64_t n,
                                    const int64_t* ids, mi_stream_t stream);
/* torch.optim.Adam's dense update (the arithmetic of mi_adam_dense_f32, bit for bit) over a list of parameter tensors of any
 * sizes — a featured model's tables, Linear, layers and scorer bias after the gradients above: tensors of 64 Ki elements or
 * more that are float4-addressable take mi_adam_dense_f32's kernel, the others share one multi-tensor launch per
 * MI_RANKER_MAX_PARAMS of them.  `step` counts from 1.  Every pointer is checked before anything is enqueued. */
int    mi_adam_multi_f32(const mi_ranker_param* params, int32_t n_params, double lr, double beta1, double beta2, double eps,
                         int64_t step, mi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * N5  PinSAGE item feature projector: bag-of-words text columns (additive to ABI 14).
 * replaces: BagOfWords / BagOfWordsPretrained (pinsage/layers.py:39-44, 49-87, 110-113): the mean of one embedding row per
 *           token of an item's text.  The third input kind of the LinearProjector, beside mi_item_projector's two.
 * A text column is a CSR over items: ptr[c] int64 [n_items + 1], tok[c] int32 [ptr[c][n_items]] with 0 <= token < vocab[c]
 * (UNCHECKED here; pad tokens are not stored), tables[c] float [vocab[c], width].
 * Forward, for output row r (item i = ids ? ids[r] : r) and column c in column order, len = ptr[c][i + 1] - ptr[c][i]:
 *     bag_c = (( E_c[tok[p0]] + E_c[tok[p0 + 1]] ) + ... ) / (float)len      one f32 chain in ascending position, then a
 *     correctly rounded division; len == 0: bag_c = 0.
 *     accumulate = 1:  out[r] = (out[r] + bag_0) + bag_1 ...   (continues mi_pinsage_project_f32's chain, text last)
 *     accumulate = 0:  out[r] =  bag_0 + bag_1 ...
 * Backward, given g = dL/d out [n, width]: g_tables[c][v] is WRITTEN with the sum over every reference (r, position) whose
 * token is v of g[r] / (float)len(i_r) (the division per reference, before the sum); rows of tokens nobody references are
 * not touched (the caller keeps the buffers zero).  The scheme of mi_pinsage_project_bwd_f32: a stable radix sort of the
 * (column, token) keys with the reference's row as payload (references in (column, r, position) order), 64-reference
 * chunks summed in order with several row loads in flight, the chunk partials of a run combined in chunk order by one
 * writer.  No float atomics: two calls give the same bits.
 * The number of references of a call (the sum of the selected items' lengths over the columns) is data-dependent: it is
 * computed on the device and the host never waits for it.  The caller passes an upper bound n_ref_max, which sizes the
 * workspace (MI_ERR_WORKSPACE, nothing enqueued, if ws_bytes is below mi_pinsage_text_bwd_workspace_bytes(p, n, n_ref_max)).
 * After the call the first int64 of ws holds the actual count; a count above n_ref_max means the bound was not one: the
 * references beyond it were dropped (nothing is written out of bounds).
 * mi_pinsage_text_clear_f32 zeroes again the rows the backward wrote for the same (n, ids).
 * width % 4 == 0, 4 <= width <= 512 (wider than a model's hidden: the one-time pooling of pretrained word vectors is this
 * forward at width = their dimension), 1 <= n_text <= MI_PROJECTOR_MAX_TEXT (MI_ERR_UNSUPPORTED otherwise); tables, out, g
 * and the gradient buffers 16-byte aligned, ptr 8-byte, tok 4-byte, ldo / ldg % 4 == 0.  Everything is validated before
 * anything is enqueued.
 * ---------------------------------------------------------------------------------- */
#define MI_PROJECTOR_MAX_TEXT 4
typedef struct mi_text_columns {
    int32_t width, n_text;
    int64_t n_items;
    const int64_t* ptr[MI_PROJECTOR_MAX_TEXT];
    const int32_t* tok[MI_PROJECTOR_MAX_TEXT];
    const float*   tables[MI_PROJECTOR_MAX_TEXT];    /* tables[c]: [vocab[c], width] */
    int64_t        vocab[MI_PROJECTOR_MAX_TEXT];
} mi_text_columns;
int64_t mi_pinsage_text_sizeof(int32_t which);       /* sizeof of: 0 mi_text_columns (binding self-check); else -1 */
int    mi_pinsage_text_f32(const mi_text_columns* p, int64_t n, const int64_t* ids /* null = 0 .. n-1 */, float* out,
                           int64_t ldo, int32_t accumulate, mi_stream_t stream);
size_t mi_pinsage_text_bwd_workspace_bytes(const mi_text_columns* p, int64_t n, int64_t n_ref_max);
int    mi_pinsage_text_bwd_f32(const mi_text_columns* p, float* const g_tables[], int64_t n, const int64_t* ids,
                               const float* g, int64_t ldg, int64_t n_ref_max, void* ws, size_t ws_bytes,
                               mi_stream_t stream);
int    mi_pinsage_text_clear_f32(const mi_text_columns* p, float* const g_tables[], int64_t n, const int64_t* ids,
                                 mi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * N5  sparse trainer: lazy Adam for the id and text tables (additive to ABI 14).
 * replaces: pinsage/model_sparse.py — nn.Embedding(sparse=True) trained by torch.optim.SparseAdam beside a dense Adam.
 * The update of ONE table row with (summed) gradient row g, every operation one correctly rounded float32 operation, no contraction
 * (torch.optim._functional.sparse_adam written out; tests/lazy_adam_emulation.py restates it):
 *     d  = g - m            m' = m + d * c1         c1 = (float)(1 - beta1)
 *     s  = g*g - v          v' = v + s * c2         c2 = (float)(1 - beta2)
 *     q  = m' / (sqrt(v') + (float)eps)
 *     p' = p + q * ss       ss = (float)(-lr * sqrt(1 - beta2^step) / (1 - beta1^step))   in double on the host
 * A row is updated if and only if it is REFERENCED by the call, also when its summed gradient is exactly zero (its moments
 * decay and p moves); a row nobody references keeps the bits of p, m and v.  The cost of a call follows the batch, not the table.
 * lr >= 0, eps >= 0, 0 <= beta < 1, step >= 1 (counts from 1), else MI_ERR_BAD_ARG.
 *
 * mi_lazy_adam_rows_f32: table p / m / v [rows, width] (contiguous), n DISTINCT row ids (UNCHECKED: 0 <= ids[r] < rows; a
 *   repeated id would be a race), their gradient rows compactly in g [n, ldg] — what mi_pinsage_step_f32 hands back through
 *   rows_out for blocks[0].src_ids: no table-sized gradient exists.  One lane per float4.  width % 4 == 0, 4 <= width <= 512
 *   (MI_ERR_UNSUPPORTED otherwise); p, m, v, g 16-byte aligned, ldg >= width, ldg % 4 == 0, 0 <= n <= rows.  No workspace.
 * mi_pinsage_project_bwd_lazy_f32: mi_pinsage_project_bwd_f32 (the same code, the same bits in every gradient buffer), then,
 *   for every slot — categorical column c, the id table — that has a moment pair in `moments`, the update above on every table
 *   row the call references, from its summed row in the slot's gradient buffer, which reads ZERO again afterwards (the store is
 *   fused: no clear is needed for that slot).  The slot's table in `p` is WRITTEN (const in the descriptor only because the other
 *   entries read it).  A slot with a null pair is left exactly as mi_pinsage_project_bwd_f32 leaves it.  moments = null or all
 *   pairs null: that call bit for bit (`lazy` is then not read).  Workspace: mi_pinsage_project_bwd_workspace_bytes(p, n).
 * mi_pinsage_text_bwd_lazy_f32: the same over mi_pinsage_text_bwd_f32; m_tables[c] / v_tables[c] both null or both set per
 *   column.  The padding slots past the device-side reference count never update a row.  n_ref_max MUST be a true upper bound
 *   of the reference count here: where the count exceeds it the plain entry leaves truncated sums the caller can still
 *   discard, this one has already applied them to p / m / v.
 *   Workspace: mi_pinsage_text_bwd_workspace_bytes(p, n, n_ref_max).
 * Everything is validated before anything is enqueued.  No float atomics; equal bits on every run.
 * ---------------------------------------------------------------------------------- */
typedef struct mi_lazy_adam {
    double  lr, beta1, beta2, eps;
    int64_t step;                                    /* of THIS update, counts from 1 */
} mi_lazy_adam;
typedef struct mi_item_projector_moments {          /* per slot both or neither; each with the shape of its table */
    float* m_tables[MI_PROJECTOR_MAX_COLS];
    float* v_tables[MI_PROJECTOR_MAX_COLS];
    float* m_id_table;
    float* v_id_table;
} mi_item_projector_moments;
int64_t mi_lazy_adam_sizeof(int32_t which);          /* sizeof of: 0 mi_lazy_adam, 1 mi_item_projector_moments; else -1 */
int    mi_lazy_adam_rows_f32(int64_t rows, int32_t width, float* p, float* m, float* v, int64_t n, const int64_t* ids,
                             const float* g, int64_t ldg, const mi_lazy_adam* lazy, mi_stream_t stream);
int    mi_pinsage_project_bwd_lazy_f32(const mi_item_projector* p, const mi_item_projector_grads* grads,
                                       const mi_item_projector_moments* moments, const mi_lazy_adam* lazy, int64_t n,
                                       const int64_t* ids, const float* g, int64_t ldg, void* ws, size_t ws_bytes,
                                       mi_stream_t stream);
int    mi_pinsage_text_bwd_lazy_f32(const mi_text_columns* p, float* const g_tables[], float* const m_tables[],
                                    float* const v_tables[], const mi_lazy_adam* lazy, int64_t n, const int64_t* ids,
                                    const float* g, int64_t ldg, int64_t n_ref_max, void* ws, size_t ws_bytes,
                                    mi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * N5  recent-items recommender (additive to ABI 14; csrc/recent_items.hip).
 * replaces: nothing in the reference.  pinsage/evaluation.py:18-53 (LatestNNRecommender) represents a user by the LAST item
 *           of their row; the PinSAGE paper serves a user from several recent pins.  These three entries are the layer
 *           between "a user's row" and "K items" for that: the user's last n_recent DISTINCT items, pooled either before
 *           the top-K (mean) or after one top-K per slot (max).  Rows are in transaction order (the rule of
 *           LatestNNRecommender); per-edge timestamps are not supported.
 * The rule, restated in numpy by tests/recent_items_emulation.py:
 *   history   The window of user u is the last min(len, 64) entries of row u; position p = 0 is the last entry.  The entry at
 *             position p is kept iff no position p' < p of the window holds the same item (distinct items, the most recent
 *             occurrence wins).  The kept entries in ascending p fill slots r = 0 .. n_slots[u] - 1, at most n_recent of
 *             them: slot 0 is the latest item, n_slots[u] >= 1 for a row with an entry.  items is slot-major
 *             [n_recent, n_users] (items[r] is a vector of query ids); unused slots hold the slot-0 item and never
 *             contribute.  An empty row gets n_slots = 0 and item 0 in every slot (the Python layer refuses such graphs).
 *   weights   w[r] = (float)pow((double)decay, r), computed by the caller: a device table of n_recent (n_lists) floats.
 *   mean      acc = 0, W = 0; for r ascending over the user's slots: p = w[r] * h[item_r][c], acc = acc + p, W = W + w[r],
 *             every operation one float32 rounding (no contraction); q[u][c] = acc / W, correctly rounded.  The answer is
 *             the top-K of q[u] . h[i] with the user's row excluded.  n_slots[u] is clamped to 1 .. n_recent.
 *   max       every slot r retrieves its own list: the top k_in of h[items[r][u]] . h[i], the user's row excluded, with
 *             scores.  The candidates of user u are the entries of lists r < n_slots[u] whose id is not -1; an item's score
 *             is the maximum over those entries of (w[r] * score) + 0.0f (one float32 multiply; the addition turns -0 into
 *             +0); the answer is the k_out candidates by (score desc, id asc), -1 / -inf pads when fewer exist.  The
 *             definition is the procedure.  For decay == 1 it is the exact top-K of max_r h[item_r] . h[i] over the
 *             eligible items: whatever outranks item i in the list of its arg-max slot also outranks it in the result.
 * mi_recent_items: one wavefront per user, no atomics, one writer per output.  ui_ptr / ui_idx: the user -> item CSR,
 *   1 <= n_recent <= MI_RECENT_MAX_SLOTS; items_out int64 [n_recent, n_users], n_slots_out int32 [n_users].
 * mi_pool_recent_f32: q_out [n_users, d] (leading dimension ldq) from table rows of leading dimension ld; d % 4 == 0, table
 *   and q_out 16-byte aligned, ld and ldq multiples of 4 and >= d.
 * mi_topk_merge_max_f32: ids int64 / scores float32 [n_lists][n_q][k_in], ids below 2^31 or -1; out_ids int64 [n_q, k_out],
 *   out_scores (nullable) float32 [n_q, k_out].  One workgroup per user sorts the entries twice in LDS, sized by the padded
 *   entry count: n_lists * k_in <= 4096, k_out <= k_in.  No float atomics, no global scratch: two calls give equal bits.
 * Returned before anything is enqueued: MI_ERR_BAD_ARG (n_recent / n_lists / k_in / k_out < 1, k_out > k_in, a negative
 *   count, a null or misaligned pointer, a leading dimension below d), MI_ERR_UNSUPPORTED (n_recent > MI_RECENT_MAX_SLOTS,
 *   d % 4 != 0, n_lists * k_in > 4096), MI_ERR_TOO_LARGE (2^31 users or more).  Zero users: 0, nothing enqueued.
 * ---------------------------------------------------------------------------------- */
#define MI_RECENT_MAX_SLOTS 16
int    mi_recent_items(int64_t n_users, const int32_t* ui_ptr, const int32_t* ui_idx, int32_t n_recent, int64_t* items_out,
                       int32_t* n_slots_out, mi_stream_t stream);
int    mi_pool_recent_f32(int64_t n_users, int32_t n_recent, int64_t d, const int64_t* items, const int32_t* n_slots,
                          const float* w, const float* table, int64_t ld, float* q_out, int64_t ldq, mi_stream_t stream);
int    mi_topk_merge_max_f32(int64_t n_q, int32_t n_lists, int32_t k_in, int32_t k_out, const int64_t* ids, const float* scores,
                             const int32_t* n_slots, const float* w, int64_t* out_ids, float* out_scores, mi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * bf16 layer tables of the LightGCN forward (opt-in: LightGCNTrainer(layer_dtype="bf16"); csrc/spmm_bf16.hip).
 * LightGCN is linear: its backward never reads a forward activation.  A step may therefore keep the LAYERS of its forward in
 * bf16 — every gathered row is then 2 d bytes instead of 4 d — and change nothing else: f32 master table, f32 read-out and
 * loss, the f32 backward products, the f32 Adam.
 *
 * The rule.  rn = round to nearest even, f32 -> bf16.  K layers, c = 1 / (K + 1):
 *   X_0      = rn(E0)                                                bf16 image of the f32 table, made once per step
 *   acc_k[r] = sum over the entries p of row r of val[p] * float(X_{k-1}[col[p]])          f32, k = 1..K
 *   X_k      = rn(acc_k)                                             stored in bf16 for k = 1..K-1 only; X_K is never stored
 *   final    = c * (E0 + float(X_1) + ... + float(X_{K-1}) + acc_K)  f32, added in this order
 * The read-out adds the STORED (rounded) layers and the unrounded last one, so that the dense step and the sparse-batch step,
 * which can only re-read what was stored, compute the same value.
 * Sums.  A short row (no plan, or at most plan->chunk entries) is ONE f32 chain acc = fmaf(val, x, acc) per output element, in
 * list order, from 0.  A split row is one such chain per work item of the plan; the partial f32 rows go to the workspace and a
 * fix-up adds them in a fixed order that depends on the row's slots alone (as in mi_spmm_csr_f32).  No float atomic anywhere;
 * two runs give equal bits; the row-list form gives the dense form's bits on the listed rows (up to the sign of zero).
 * Gradient.  The backward of a step that runs this forward is today's f32 one, that of the UNROUNDED linear map: the rounding is
 * treated as the identity (straight-through).
 *
 * mi_rows_f32_to_bf16: dst[r, :] = rn(src[r, :]), one pass with the hardware's packed conversion.  d % 8 == 0; src / dst
 *   16-byte aligned, ld_src a multiple of 4 floats, ld_dst a multiple of 8 elements, both >= d.  +-0 and +-inf map to
 *   themselves, a finite value beyond the largest bf16 rounds to inf; NaN is outside the contract.
 * mi_spmm_csr_bf16: the product above.  X and the optional Y are bf16 rows (uint16 bit patterns), val, addend and S f32:
 *     if (Y) Y[r, :] = rn(acc)
 *     if (S) S[r, :] = scale * ((addend ? addend[r, :] : 0) + (Y ? float(rn(acc)) : acc))
 *   d % 8 == 0 and d <= 256; ldx / ldy multiples of 8 elements, lda / lds of 4 floats, all >= d; rows 16-byte aligned.  S may
 *   alias addend; Y and S must not alias X.  A row is a sub-group of max(4, the power of two >= d / 8) lanes, a lane loads 16
 *   bytes = 8 elements of a row and keeps 8 f32 sums: at d = 128 one wave-instruction fetches four neighbour rows.
 *   row_list / n_list_dev / n_list: as in mi_spmm_ex (Y, S and addend compact by list position; needs plan->long_index when
 *   the plan has split rows); rows at and beyond *n_list_dev are not written.  parts: 0 = the whole product, or a mask of
 *   MI_SPMM_SHORT_ROWS / MI_SPMM_SPLIT_ROWS (disjoint output rows: the halves may run on two streams).
 *   plan: null, or a WORK-ITEM plan as mi_spmm_plan_fill writes it (items in launch order, negative slots = padding, long_rows,
 *   item_ptr, long_index).  epos / ecol / eval are not read: val comes from the CSR arrays for every entry, so a re-weighted
 *   adjacency needs no copy refreshed.  ws: mi_spmm_workspace_bytes(plan, d).  The sweep form, thin rows and the hot, sliced
 *   and persistent short-row launches do not exist here: do not pass a plan counted with thin rows or laid out as a sweep.
 * mi_gather_rows_bf16_f32: dst[i, :] = (accumulate ? dst[i, :] : 0) + float(src[rows[i], :]) for i < min(n_max, n_dev ? *n_dev
 *   : n_max) — the running layer sum at the batch's rows.  d % 8 == 0, alignments as above.
 * Returned before anything is enqueued: MI_ERR_BAD_ARG (a width that is no multiple of 8, a null or misaligned pointer, a bad
 *   leading dimension, Y or S on X, an unknown bit in parts, a plan with work items but without its arrays),
 *   MI_ERR_UNSUPPORTED (mi_spmm_csr_bf16 with d > 256), MI_ERR_WORKSPACE (ws null or short), MI_ERR_TOO_LARGE (2^31 rows).
 * ---------------------------------------------------------------------------------- */
int mi_rows_f32_to_bf16(int64_t n_rows, int64_t d, const float* src, int64_t ld_src, uint16_t* dst, int64_t ld_dst,
                        mi_stream_t stream);
int mi_spmm_csr_bf16(int64_t n_rows, int64_t d,
                     const int32_t* rowptr, const int32_t* col, const float* val,
                     const uint16_t* X, int64_t ldx,
                     uint16_t* Y, int64_t ldy,
                     const float* addend, int64_t lda,
                     float* S, int64_t lds, float scale,
                     const mi_spmm_plan* plan,
                     const int32_t* row_list, const int32_t* n_list_dev, int64_t n_list, int32_t parts,
                     void* ws, size_t ws_bytes, mi_stream_t stream);
int mi_gather_rows_bf16_f32(int64_t n_max, const int32_t* n_dev, int64_t d, const int32_t* rows,
                            const uint16_t* src, int64_t ld_src, float* dst, int64_t ld_dst, int32_t accumulate,
                            mi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * iALS  implicit-feedback ALS row solves (additive to ABI 14; csrc/als.hip).
 * replaces: nothing in the reference.  Implicit-feedback matrix factorisation by alternating least squares (Hu, Koren and
 *           Volinsky, ICDM 2008; Rendle et al., RecSys 2022) is the trained baseline a LightGCN figure is read against: with
 *           one table fixed, every row of the other is the solution of one d x d system built from the row's entries.  This
 *           entry is that half-sweep, and — on any other CSR over the same table — the fold-in of rows the model never saw.
 * Inputs.  A CSR (ptr int32 [n_rows + 1], idx int32 [nnz]) over a factor table Y [n_cols, d] (f32, leading dimension ldy >= d),
 *   G [d, d] (f32, contiguous, symmetric: only G[j][k] with k <= j is read; the trainer passes Y^T Y), alpha >= 0, reg > 0.
 * The rule, per row r with entries e_0 .. e_{n-1} in CSR order (y_e = Y[idx[e], :]), restated in float64 by
 * tests/als_emulation.py:
 *   chunks    Chunk c is entries [c L, (c + 1) L) of the row, L = mi_als_chunk(d): a compile-time constant of d alone (not of
 *             the device, the grid or the other rows).
 *   per chunk S_c[j][k] = sum_e y_e[j] * y_e[k], ONE chain acc = fmaf(y_e[j], y_e[k], acc) from 0 in entry order;
 *             s_c[j] = sum_e y_e[j], acc = acc + y_e[j] from 0 in entry order.
 *   across    S = ((S_0 + S_1) + S_2) ... in ascending c, one f32 addition each; s likewise.
 *   system    A[j][k] = fmaf(alpha, S[j][k], G[j][k]), then reg added on the diagonal (A[j][j] = fmaf(..) + reg);
 *             b[j] = (1.0f + alpha) * s[j].
 *   solve     x_r solves A x = b by an f32 Cholesky factorisation (A = L L^T, forward then backward substitution).  The order of
 *             the additions inside the factorisation and the substitutions is the kernel's and NOT part of the rule; the tests
 *             bound the residual instead (tests/als_emulation.py: residual_bound).
 *   empty row x_r = 0.
 *   pivot     A pivot that is not a positive finite number: x_r = 0 and *n_failed is incremented by one (an int32 device
 *             counter the CALLER zeroes; an integer atomic).  Nothing is read or written out of bounds on that path.
 * Duplicates.  For duplicate-free rows this is exactly iALS with confidence 1 + alpha on the observed pairs and 1 on all
 *   others.  A repeated entry is summed as written, i.e. counts once per occurrence in S and in s.
 * No float atomics anywhere: two calls give equal bits, and a row's answer is a pure function of (its entries in order, Y, G,
 *   alpha, reg) whatever else is in the call — alone, in a batch, through row_list.
 * row_list / n_list: null, or n_list int32 row ids (any order; distinct); X is then COMPACT by list position (X[i, :] belongs to
 *   row row_list[i]).  An id outside [0, n_rows) gives a zero row.  Without a list X[r, :] belongs to row r.  X: f32, leading
 *   dimension ldx >= d.
 * Guards.  idx[e] outside [0, n_cols) contributes a zero row y_e.  A rowptr that runs past nnz, or a long row that found no
 *   workspace slot (possible only when row_list names a row twice), is treated as a failed pivot: zero row, counted.
 * Workspace: mi_als_solve_rows_workspace_bytes(n_work, nnz, d), n_work = n_list with a list and n_rows without:
 *   (d * d + d) * 4 bytes for each of at most nnz / L + nnz / (L + 1) chunks of rows longer than L, and 8 bytes per row.
 * Returned before anything is enqueued: MI_ERR_BAD_ARG (d % 4 != 0 — rows are read as float4 —, d < 4 or d > 128, 2^31 or
 *   more rows, columns or entries, a negative count, alpha < 0 or not finite, reg <= 0 or not finite, a null pointer, Y not
 *   16-byte aligned, ldy % 4 != 0, ldy < d or ldx < d), MI_ERR_WORKSPACE (ws null or short).  Zero rows: 0, nothing enqueued.
 * mi_als_chunk: L of a width, 0 for a width the entry refuses.
 * ---------------------------------------------------------------------------------- */
int32_t mi_als_chunk(int64_t d);
size_t  mi_als_solve_rows_workspace_bytes(int64_t n_work, int64_t nnz, int64_t d);
int     mi_als_solve_rows_f32(int64_t n_rows, int64_t d, const int32_t* ptr, const int32_t* idx, int64_t nnz, int64_t n_cols,
                              const float* Y, int64_t ldy, const float* G, float alpha, float reg, float* X, int64_t ldx,
                              const int32_t* row_list, int64_t n_list, int32_t* n_failed, void* ws, size_t ws_bytes,
                              mi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * iALS block  implicit-feedback ALS, block row solver (additive to ABI 14; csrc/als_block.hip).
 * replaces: nothing in the reference.  The iALS entry above forms and factorises one d x d system per row; this entry
 *           minimises the same row quadratic 1/2 x^T A x - b^T x (A and b of the iALS entry) exactly over one block of
 *           B coordinates at a time, as iALS++ does (Rendle, Krichene, Zhang and Koren, RecSys 2021): the largest system is
 *           B x B, the width goes to 256, and a row of n entries costs about 2 n d B + 2 d^2 + d B^2 / 3 flop per sweep.
 *           It is a ROW-LOCAL variant.  The paper's outer loop runs over blocks, with all users and then all items inside
 *           it, and keeps the predictions of all pairs in memory between steps; here a half-sweep walks all blocks of one row
 *           before the next row, which makes it one launch, and the predictions p_e never outlive the row's wavefront.
 * Inputs.  As the iALS entry: a CSR over Y [n_cols, d] (ldy), G [d, d] of which only G[j][k] with k <= j is read
 *   (G(j, k) below is G[max(j, k)][min(j, k)]), alpha >= 0, reg > 0; and block B in {16, 32, 64}, sweeps in 1 .. 64, from_zero.
 *   X [n_work, d] (ldx) is IN/OUT: a row starts from its current content of X (from the place its result goes to, i.e. by list
 *   position with a row_list), or from 0 when from_zero is not 0 (X is then not read).
 * The rule, per row r with entries e_0 .. e_{n-1} in CSR order (y_e = Y[idx[e], :]) and start x, restated in float64 and in
 * float32 by tests/als_block_emulation.py.  "dot16(u, v, m)" for vectors over m columns is: 16 chains t_c, c = 0 .. 15,
 * t_c = fmaf(u[c + 16 i], v[c + 16 i], t_c) from 0 over i ascending while c + 16 i < m, then added pairwise as a tree at
 * distances 8, 4, 2, 1 (t_c + t_{c ^ 8}, ...).
 *   start     p_e = dot16(y_e, x, d) for every entry; exactly 0 under from_zero.
 *   for t in 0 .. sweeps-1, for c in 0 .. ceil(d / B)-1, pi = [c B, min((c + 1) B, d)) (the last block may be partial):
 *     w_e     = fmaf(alpha, p_e, -(1.0f + alpha))
 *     q[j]    = sum_k G(j, k) x[k], j in pi, over ALL k < d, from the CURRENT x: 64 / B chains, chain m = fmaf(G(j, k), x[k],
 *               acc) from 0 over the groups of four columns k = 4 u .. 4 u + 3, u = m, m + 64 / B, .. ascending, the chains
 *               added in ascending m.
 *     gs[j]   = sum_e w_e y_e[j], ONE chain acc = fmaf(y_e[j], w_e, acc) from 0 over ALL the row's entries in order.
 *     g[j]    = fmaf(reg, x[j], gs[j] + q[j])
 *     S[j][k] = sum_e y_e[j] y_e[k], ONE chain acc = fmaf(y_e[j], y_e[k], acc) from 0 over ALL the row's entries in order;
 *     H[j][k] = fmaf(alpha, S[j][k], G(j, k)), + reg on the diagonal (H[j][j] = fmaf(..) + reg),   j, k in pi
 *     delta   solves H delta = -g by an f32 Cholesky of the |pi| x |pi| system; the order inside it is the kernel's and NOT part
 *               of the rule.
 *     x[j]    = x[j] + delta[j], j in pi;   p_e = p_e + dot16(y_e[pi], delta, |pi|)   (not after the very last step)
 *   There are no chunks in any sum: a row is walked by one wavefront, so the order is a function of (the row's entries in
 *   order, d, B, sweeps) alone, never of the device, the grid or the other rows.  mi_als_block_chunk(d, B) is the one
 *   constant that changes the kernel's PATH: a row of at most that many entries keeps its factor rows and p_e on chip, a
 *   longer one re-gathers its block columns per block and keeps p_e in the workspace, by entry position.  Both paths run
 *   the sums above in the same order and give the same bits.
 *   empty row x_r = 0 (also with a start).
 *   pivot     A pivot that is not a positive finite number, in any block step: x_r = 0 and *n_failed is incremented by one (an
 *             int32 device counter the CALLER zeroes; an integer atomic).
 * No float atomics anywhere: two calls give equal bits, and a row alone gives the bits it has in a batch or through row_list.
 * row_list / n_list: as the iALS entry (distinct ids; X compact by list position; an id outside [0, n_rows) gives a zero row).
 * Guards.  idx[e] outside [0, n_cols) contributes a zero row y_e.  A rowptr that runs past nnz is treated as a failed pivot.
 * Workspace: mi_als_block_rows_workspace_bytes(n_work, nnz, d, block) = d * d * 4 bytes (G(j, k) written out as a full
 *   matrix by a first small kernel) and 4 bytes per entry (at least one), each rounded up to 256.
 * Returned before anything is enqueued: MI_ERR_BAD_ARG (d % 4 != 0, d < 4 or d > 256, block not 16, 32 or 64, sweeps outside
 *   1 .. 64, and everything the iALS entry refuses), MI_ERR_WORKSPACE (ws null or short).  Zero rows: 0, nothing enqueued.
 * mi_als_block_chunk: 0 for a shape the entry refuses.
 * ---------------------------------------------------------------------------------- */
int32_t mi_als_block_chunk(int64_t d, int64_t block);
size_t  mi_als_block_rows_workspace_bytes(int64_t n_work, int64_t nnz, int64_t d, int64_t block);
int     mi_als_block_rows_f32(int64_t n_rows, int64_t d, int64_t block, int64_t sweeps, const int32_t* ptr,
                              const int32_t* idx, int64_t nnz, int64_t n_cols, const float* Y, int64_t ldy, const float* G,
                              float alpha, float reg, float* X /* in/out */, int64_t ldx, int32_t from_zero,
                              const int32_t* row_list, int64_t n_list, int32_t* n_failed, void* ws, size_t ws_bytes,
                              mi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * iALS weighted  the iALS entry with a confidence per entry and a regulariser per row (additive to ABI 14; csrc/als.hip).
 * replaces: nothing in the reference.  Hu, Koren and Volinsky's c_ui = 1 + alpha r_ui (the caller passes a_e = alpha r_e) and
 *           the frequency-scaled regulariser of Rendle et al. (RecSys 2022, section 4) as a value per row.  The iALS entry
 *           above keeps its signature, its code and its bits; this one solves, per row r,
 *               (G + sum_e a_e y_e y_e^T + reg_r I) x = sum_e (1 + a_e) y_e.
 * Inputs.  As the iALS entry, with `conf` [nnz] (f32; a_e by ENTRY POSITION in idx) in the place of alpha and
 *   `reg_rows` [n_rows] (f32; indexed by ROW ID, never by list position; null = the scalar `reg` for every row).
 *   a_e must be finite and >= 0; the entry does not scan conf.
 * The rule, per row r with entries e in CSR order, y_e = Y[idx[e], :], a_e = conf[e], c_e = 1.0f + a_e (one rounding),
 * reg_r = reg_rows ? reg_rows[r] : reg; restated in float64 and float32 by tests/als_weighted_emulation.py:
 *   z         z_e[k] = a_e * y_e[k], ONE f32 product per element.
 *   chunks    As the iALS entry: chunk c is entries [c L, (c + 1) L) of the row, L = mi_als_chunk(d).
 *   per chunk S_c[j][k] = ONE chain acc = fmaf(y_e[j], z_e[k], acc) from 0 in entry order, for k <= j (the row index is
 *             the y side, the column index the z side);  s_c[j] = ONE chain acc = fmaf(c_e, y_e[j], acc) from 0 in entry order.
 *   across    S = ((S_0 + S_1) + S_2) ... in ascending c, one f32 addition each; s likewise.
 *   system    A[j][k] = G[j][k] + S[j][k] (one addition), then reg_r added on the diagonal (A[j][j] = (G + S) + reg_r);
 *             b[j] = s[j].
 *   solve, empty row, pivot: as the iALS entry.
 *   reg_r     A reg_rows[r] that is not a positive finite number makes row r a failed row: x_r = 0, counted in *n_failed; an
 *             EMPTY row is zero and not counted whatever its reg_rows.
 *   conf      A negative or non-finite a_e may cost the row its definiteness and is then handled by the pivot rule (zero row,
 *             counted); a NaN that reaches x is the caller's.  Nothing is read or written out of bounds on any such input.
 * Duplicates, determinism, row_list / n_list, guards, workspace (mi_als_solve_rows_w_workspace_bytes, the same size and
 *   layout): as the iALS entry; with a row_list, conf is still by entry position and reg_rows by row id.
 * Returned before anything is enqueued: everything the iALS entry refuses (alpha apart), MI_ERR_BAD_ARG for a null conf, and
 *   for reg <= 0 or not finite when reg_rows is null (with reg_rows given, reg is not looked at).
 * ---------------------------------------------------------------------------------- */
size_t  mi_als_solve_rows_w_workspace_bytes(int64_t n_work, int64_t nnz, int64_t d);
int     mi_als_solve_rows_w_f32(int64_t n_rows, int64_t d, const int32_t* ptr, const int32_t* idx, int64_t nnz,
                                int64_t n_cols, const float* Y, int64_t ldy, const float* G, const float* conf,
                                const float* reg_rows /* nullable */, float reg, float* X, int64_t ldx,
                                const int32_t* row_list, int64_t n_list, int32_t* n_failed, void* ws, size_t ws_bytes,
                                mi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * iALS block weighted  the iALS block entry with the same two additions (additive to ABI 14; csrc/als_block.hip).
 * Minimises the row quadratic of the "iALS weighted" entry, 1/2 x^T A x - b^T x, over one block of B coordinates at a time.
 * Inputs.  As the iALS block entry, with conf [nnz] and reg_rows [n_rows] (nullable) as in the iALS weighted entry.
 * The rule is the "iALS block" rule with these changes (a_e = conf[e], c_e = 1.0f + a_e, reg_r as above), restated in
 * float64 and float32 by tests/als_weighted_emulation.py:
 *     w_e     = fmaf(a_e, p_e, -c_e)
 *     g[j]    = fmaf(reg_r, x[j], gs[j] + q[j])            (gs and q as in the iALS block rule, gs with this w_e)
 *     S[j][k] = ONE chain acc = fmaf(y_e[j], z_e[k], acc) from 0 over ALL the row's entries in order, z_e[k] = a_e * y_e[k]
 *               (one f32 product), k <= j
 *     H[j][k] = G(j, k) + S[j][k] (one addition), + reg_r on the diagonal,   j, k in pi
 *   Start, q, delta, the update of x and p_e, the absence of chunks, the empty row and the pivot rule are unchanged.  A row of
 *   at most min(mi_als_block_chunk(d, B), 128) entries (the 128 binds at d <= 16 only) keeps a_e on chip beside p_e; a longer
 *   one re-reads conf with every streamed piece (conf is not copied into the workspace).  Both paths give the same bits.
 *   A reg_rows[r] that is not a positive finite number: a failed row (zero, counted), as in the iALS weighted entry.
 * Workspace: mi_als_block_rows_w_workspace_bytes, the size of the iALS block entry's.
 * Returned before anything is enqueued: everything the iALS block entry refuses (alpha apart), a null conf, and reg <= 0 or
 *   not finite when reg_rows is null.
 * ---------------------------------------------------------------------------------- */
size_t  mi_als_block_rows_w_workspace_bytes(int64_t n_work, int64_t nnz, int64_t d, int64_t block);
int     mi_als_block_rows_w_f32(int64_t n_rows, int64_t d, int64_t block, int64_t sweeps, const int32_t* ptr,
                                const int32_t* idx, int64_t nnz, int64_t n_cols, const float* Y, int64_t ldy, const float* G,
                                const float* conf, const float* reg_rows /* nullable */, float reg, float* X /* in/out */,
                                int64_t ldx, int32_t from_zero, const int32_t* row_list, int64_t n_list, int32_t* n_failed,
                                void* ws, size_t ws_bytes, mi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * iALS block hub  the two iALS block entries with hub rows taken from an assembled system (additive to ABI 14;
 *                 csrc/als_block.hip, the Gram code shared with csrc/als.hip through csrc/als_gram.hpp).
 * replaces: nothing in the reference.  One wavefront walks a row in the block entries, so a row of half a million entries
 *           is a half-sweep of its own.  For n >> d the block form's 2 n d B flop per block times d / B blocks IS the full
 *           Gram: here a row with MORE THAN hub_threshold entries has its d x d system formed once, over one workgroup per
 *           chunk of its entries, and the block steps run on that system.  Every other row is the block entry's, bit for bit.
 * Inputs.  As the iALS block entry (the _w_ pair: as the iALS block weighted entry), and hub_threshold >= 1, n_hub_rows,
 *   n_hub_chunks: the caller's counts, over the rows the call works on, of the rows with n > hub_threshold entries and of
 *   sum ceil(n / L_h) over them (counts over the whole CSR are upper bounds for a row_list of distinct rows).
 * The rule for a hub row r (entries e in CSR order, y_e, a_e, c_e, reg_r as in the entries named), restated in float64 and
 * float32 by tests/als_hub_emulation.py:
 *   chunks    Chunk c is entries [c L_h, (c + 1) L_h) of the row, L_h = mi_als_block_hub_chunk(d): a compile-time constant
 *             of d alone (256 up to d = 64, 512 beyond: shorter than the iALS entry's L, because a hub row's answer is as
 *             good as its Gram — the block rule refines through p_e, this one cannot — and a chain's error grows with its
 *             length).
 *   per chunk S_c[j][k], k <= j, ONE fmaf chain from 0 in entry order, and s_c[j], one chain from 0 in entry order: exactly
 *             the "per chunk" line of the iALS entry, and for the _w_ pair of the iALS weighted entry (z_e = a_e * y_e,
 *             S_c[j][k] = chain of fmaf(y_e[j], z_e[k], acc); s_c[j] = chain of fmaf(c_e, y_e[j], acc), c_e = 1.0f + a_e).
 *   across    S = ((S_0 + S_1) + S_2) ... in ascending c, one f32 addition each; s likewise.
 *   system    exactly the "system" line of the iALS entry (A[j][k] = fmaf(alpha, S[j][k], G[j][k]), + reg on the diagonal,
 *             b[j] = (1.0f + alpha) * s[j]) or of the iALS weighted entry (A = G + S, + reg_r on the diagonal, b = s), for
 *             k <= j;  A(j, k) below is A[max(j, k)][min(j, k)].
 *   start     x from X, or 0 under from_zero, as in the block entry.
 *   for t in 0 .. sweeps-1, for c in 0 .. ceil(d / B)-1, pi = [c B, min((c + 1) B, d)):
 *     u[j]    = sum_k A(j, k) x[k], j in pi, over ALL k < d, from the CURRENT x, in the chain layout of the block rule's q:
 *               64 / B chains, chain m = fmaf(A(j, k), x[k], acc) from 0 over the groups of four columns k = 4 u .. 4 u + 3,
 *               u = m, m + 64 / B, .. ascending, the chains added in ascending m.
 *     g[j]    = u[j] - b[j]
 *     H       = A[pi, pi]
 *     delta   solves H delta = -g by an f32 Cholesky whose inner order is the kernel's and NOT part of the rule.
 *     x[j]    = x[j] + delta[j], j in pi
 *   In exact arithmetic this is the block rule's own iteration (p_e = y_e . x, so sum_e w_e y_e + G x + reg x = A x - b).
 *   empty row, pivot, reg_rows, guards (idx out of range, a rowptr that runs past nnz, n_failed): exactly the block entry's.
 *   no slot   A hub row that found no workspace slot (n_hub_rows or n_hub_chunks too small, a row listed twice) is a failed
 *             row: zero, counted.  Nothing is read or written out of bounds.
 * No float atomics.  A hub row's bits are a function of (its entries in order, Y, G, alpha or conf, reg, the start, d, B,
 *   sweeps) alone: not of the device, the grid, the other rows, row_list, or of hub_threshold beyond which side of it the row
 *   falls on.  Which workspace slot a row or a chunk gets (integer atomics) may differ from run to run; what is written into
 *   it does not.  A row with at most hub_threshold entries has the bits the iALS block (weighted) entry gives it.
 * Workspace: mi_als_block_rows_hub_workspace_bytes(n_work, nnz, d, block, n_hub_rows, n_hub_chunks) = the block entry's
 *   bytes + 256 + 4 n_work + 8 n_hub_rows + 4 n_hub_chunks + 4 n_hub_chunks (256 T + 16 ceil(d / 16)) + 4 n_hub_rows (d d + d),
 *   every term rounded up to 256, T = ceil(d / 16) (ceil(d / 16) + 1) / 2 the 16 x 16 tiles of a lower triangle: a chunk slot
 *   holds the lower triangle only, a row slot A as a full symmetric matrix and b.  It grows with the hub rows that exist.
 * Returned before anything is enqueued: everything the block entry refuses, MI_ERR_BAD_ARG for hub_threshold < 1 or a count
 *   that is negative or 2^31 or more, MI_ERR_WORKSPACE (ws null or short).  Zero rows: 0, nothing enqueued.
 * mi_als_block_hub_chunk: L_h of a width, 0 for a width the entry refuses.  The size queries return 0 for refused arguments.
 * ---------------------------------------------------------------------------------- */
int32_t mi_als_block_hub_chunk(int64_t d);
size_t  mi_als_block_rows_hub_workspace_bytes(int64_t n_work, int64_t nnz, int64_t d, int64_t block, int64_t n_hub_rows,
                                              int64_t n_hub_chunks);
int     mi_als_block_rows_hub_f32(int64_t n_rows, int64_t d, int64_t block, int64_t sweeps, const int32_t* ptr,
                                  const int32_t* idx, int64_t nnz, int64_t n_cols, const float* Y, int64_t ldy,
                                  const float* G, float alpha, float reg, float* X /* in/out */, int64_t ldx,
                                  int32_t from_zero, const int32_t* row_list, int64_t n_list, int64_t hub_threshold,
                                  int64_t n_hub_rows, int64_t n_hub_chunks, int32_t* n_failed, void* ws, size_t ws_bytes,
                                  mi_stream_t stream);
size_t  mi_als_block_rows_hub_w_workspace_bytes(int64_t n_work, int64_t nnz, int64_t d, int64_t block, int64_t n_hub_rows,
                                                int64_t n_hub_chunks);
int     mi_als_block_rows_hub_w_f32(int64_t n_rows, int64_t d, int64_t block, int64_t sweeps, const int32_t* ptr,
                                    const int32_t* idx, int64_t nnz, int64_t n_cols, const float* Y, int64_t ldy,
                                    const float* G, const float* conf, const float* reg_rows /* nullable */, float reg,
                                    float* X /* in/out */, int64_t ldx, int32_t from_zero, const int32_t* row_list,
                                    int64_t n_list, int64_t hub_threshold, int64_t n_hub_rows, int64_t n_hub_chunks,
                                    int32_t* n_failed, void* ws, size_t ws_bytes, mi_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* LAPLACE_HIP_H */
