"""Tensor-level wrappers over the C ABI (include/laplace_hip.h).

PyTorch is plumbing here: device memory, the current HIP stream, dtype/shape checks.  Every
function requires GPU tensors and raises otherwise — there is no CPU path in the product.
"""
from __future__ import annotations

import ctypes
import itertools
import math
import numbers
import os
from os import environ as _os_environ
from dataclasses import dataclass, field
from typing import Optional, Tuple

import torch as t
from torch import Tensor

from . import _lib
from ._lib import SpmmExStruct, SpmmPlanStruct, SpmmSweepStruct, check

DEFAULT_CHUNK = 256  # max nnz per work item of a split (hub) row
# columns per band of a banded work-item plan (the adjacencies the SWEEP form does not take: C4's 8 M x 100 K graph on one GPU).
# The work items of a band run together on one XCD and meet in its L2.  A/B on C4 at N = 1, round 3 (tools/ab_c4_bandwidth.sh,
# profiles/r03_c4_band_width.txt; ms per step / dense launch / sparse-operand launch): 2 048: 73.5 / 12.38 / 9.90, 4 096: 65.3 /
# 11.00 / 8.50, 8 192 (rounds 1-2: "the 4 MB L2"): 58.3 / 9.98 / 7.27, 16 384: 54.3 / 9.39 / 6.39, 32 768: 56.2 / 9.98 / 6.24,
# 65 536: 58.6 / 10.62 / 6.16, 131 072: 60.4 / 11.06 / 6.29 — fewer, longer work items (half the partial rows) outweigh the
# band outgrowing one L2 up to 8 MB of rows.  Widening only the THIN rows' bands is slower (csrc/spmm.hip, plan_seg_flags_kernel).
DEFAULT_BAND = int(_os_environ.get("LAPLACE_SPMM_BAND", 16384))
MIN_BANDED_COLS = 131072  # narrower adjacencies keep the row-major plan (nothing to block for)
# THIN rows of a default banded plan: split rows of at most THIN_PER_BAND * n_bands entries get no work items and are summed
# whole by a wavefront each (csrc/spmm.hip, spmm_thin_kernel).  Such a row holds THIN_PER_BAND entries per band at most, i.e.
# it paid a 512-byte partial row, written and read back, for every one or two gathers (C4: 58 % of the 7.7 M work items hold
# 11 % of the split rows' entries, profiles/thin_rows_c4.md).  A/B on C4 at N = 1 (same process, one graph, 20 steps after 5;
# ms per step / dense launch / sparse-operand launch): 0: 51.18, 51.57, 50.84 / 9.12 / 5.36, 1: 49.52 / 8.75 / 5.18,
# 2: 47.39, 47.55 / 8.38 / 4.99, 3: 47.57, 47.28, 4: 47.79, 47.66 / 8.52 / 5.07, 6: 48.70, 8: 49.06 / 8.66 / 5.18 — past ~4 entries per
# band the lost L2 company of the band costs more than the partial rows did.  0 = no thin rows, the plan of before.
# LAPLACE_SPMM_THIN overrides for A/B.
THIN_PER_BAND = int(_os_environ.get("LAPLACE_SPMM_THIN", 2))

# bench.py sets this to a list to collect (start, end, kind) HIP events around every propagate launch,
# recorded on the stream the kernels are launched on.  None = no timing overhead.
SPMM_EVENTS = None

# The short-row kernel of a planned product runs on a side stream beside the split-row kernels (mi_spmm_ex.parts): disjoint
# output rows, the same kernels, bitwise the single-stream result (tests/test_gpu_lightgcn.py).  Round 1, against the
# work-item form of the split rows: 1 % (step 5.855 -> 5.782 ms), left off.  Round 3, against the SWEEP form — one 1 024-thread
# workgroup per CU that is bound by its L2 -> CU gathers (profiles/r03_sweep.md) and leaves half of every CU's wavefront
# slots and the fabric to the short rows: dense launch 0.961 -> 0.902 ms, step 5.52 -> 5.34 ms on C2 (same box, bench.py
# LAPLACE_SPMM_TWO_STREAMS=0 / 1; the enqueue order of the two halves does not matter).  On by default;
# LAPLACE_SPMM_TWO_STREAMS=0 switches it off.  (2 = split rows enqueued first: an A/B setting.)
SPMM_TWO_STREAMS = int(os.environ.get("LAPLACE_SPMM_TWO_STREAMS", "1") or 0)
PACK_ENTRIES = os.environ.get("LAPLACE_SPMM_PACK", "1") != "0"   # A/B: banded plans carry launch-ordered copies of their entries
X_RARE_BITS = os.environ.get("LAPLACE_X_RARE", "1") != "0"   # A/B: spmm(..., x_rare=True) honoured (mi_spmm_ex.x_bits)
_SIDE = {}


def _side_stream(device) -> "t.cuda.Stream":
    key = t.device(device).index
    if key not in _SIDE:
        _SIDE[key] = t.cuda.Stream(device=device)
    return _SIDE[key]

# Adjacencies smaller than this run without a split-row plan (one wavefront per row whatever its
# length): building a plan reads two counters back to the host, which per-batch subgraphs of the
# ranker cannot afford and do not need.
PLAN_MIN_NNZ = 1 << 20


_stream = _lib.current_stream


def _ptr(x: Optional[Tensor]) -> Optional[int]:
    if x is None:
        return None
    return x.data_ptr() if x.numel() > 0 else None


def _need(x: Tensor, dtype: t.dtype, name: str, contiguous: bool = True) -> None:
    try:  # the valid case in three attribute reads; the messages below are for everything else
        if x.dtype is dtype and x.is_cuda and (not contiguous or x.is_contiguous()):
            return
    except AttributeError:
        pass
    if not isinstance(x, Tensor):
        raise TypeError(f"{name}: expected a tensor, got {type(x)}")
    if not x.is_cuda:
        raise _lib.MiError(f"{name}: tensor is on {x.device}; the HIP path needs a GPU tensor (no CPU fallback)")
    if x.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {x.dtype}")
    if contiguous and not x.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")


def _rows_ok(x: Tensor, name: str) -> int:
    """Checks a 2-D fp32 row-major matrix with unit inner stride; returns its leading dimension."""
    try:  # the valid case first and in one frame: this runs ~130 times per ranker iteration
        if x.dtype is t.float32 and x.is_cuda and x.dim() == 2:
            (r, c), (s0, s1) = x.shape, x.stride()
            if c <= 1 or s1 == 1:
                return s0 if r > 1 else max(c, s0)
    except AttributeError:
        pass
    _need(x, t.float32, name, contiguous=False)
    if x.dim() == 2 and x.shape[0] == 0:   # no rows (a node type absent from the batch): any strides, e.g. autograd's (0, 0)
        return max(int(x.shape[1]), 1)
    if x.dim() != 2 or (x.shape[1] > 1 and x.stride(1) != 1):
        raise ValueError(f"{name}: expected a row-major 2-D matrix, got shape {tuple(x.shape)} strides {x.stride()}")
    return x.stride(0) if x.shape[0] > 1 else max(x.shape[1], x.stride(0))


def _ws(nbytes: int, device) -> Tensor:
    return t.empty(max(int(nbytes), 256), dtype=t.uint8, device=device)


_WS_CACHE = {}


def _ws_reused(nbytes: int, device) -> Tensor:
    """Scratch for launches that consume it before they return control to the stream's next launch (the GEMM split-K
    partials): one buffer per (device, stream), grown on demand, instead of an allocation per call — the ranker issues
    ~10 such launches per iteration.  Launches on one stream run in order, so the next user cannot overtake the last."""
    dev = t.device(device) if not isinstance(device, int) else t.device("cuda", device)
    key = (dev.index if dev.index is not None else t.cuda.current_device(), _stream())
    cur = _WS_CACHE.get(key)
    if cur is None or cur.numel() < nbytes:
        cur = t.empty(max(int(nbytes) * 2, 1 << 20), dtype=t.uint8, device=dev)
        _WS_CACHE[key] = cur
    return cur


# --------------------------------------------------------------------------------------
# CSR container
# --------------------------------------------------------------------------------------
_VAL_GEN = itertools.count(1)


@dataclass
class SpmmPlan:
    struct: SpmmPlanStruct
    long_rows: Optional[Tensor]
    item_ptr: Optional[Tensor]
    items: Optional[Tensor]
    long_index: Optional[Tensor] = None
    partial: dict = field(default_factory=dict)  # d -> workspace tensor
    sweep: Optional[SpmmSweepStruct] = None       # split rows in SWEEP form (mi_spmm_sweep); tensors kept in sweep_t
    sweep_t: tuple = ()
    wide: Optional["SpmmPlan"] = None             # work-item plan of the same adjacency for widths the sweep form lacks
    packed: tuple = ()                            # (epos, ecol, eval): the split rows' entries in launch order (mi_spmm_plan_pack_entries)
    sweep_src: Optional[Tensor] = None            # int32: position in a.val of every entry of sweep_t[1] (val_s), for a re-gather
    values_of: tuple = ()                         # (source tensor, its _version, the adjacency's value generation) the
                                                  # plan's value copies (packed[2], sweep_t[1]) were taken from: _sync_plan_values
    nnz_long: int = 0
    thin_rows: Optional[Tensor] = None            # int32: rows with chunk < degree <= thin_max, longest first (mi_spmm_ex.thin_rows)
    thin_max: int = 0
    slice_reuse: dict = field(default_factory=dict)   # first hot row -> gathers per gathered column of the rows in front of it (spmm, ROW_SLICES)
    tiles: Optional["_lib.SpmmTilesStruct"] = None    # hub rows in TILES form (mi_spmm_tiles); tensors kept in tiles_t (build_hub_tiles_layout)
    tiles_t: dict = field(default_factory=dict)

    @property
    def n_thin_rows(self) -> int:
        return int(self.thin_rows.numel()) if self.thin_rows is not None else 0

    @property
    def n_split_rows(self) -> int:
        return int(self.struct.n_long_rows)

    @property
    def n_long_rows(self) -> int:
        """Rows with more than `chunk` entries, i.e. not the short-row kernel's: the split rows and the thin rows."""
        return int(self.struct.n_long_rows) + self.n_thin_rows

    @property
    def n_items(self) -> int:
        return int(self.struct.n_items)


@dataclass
class DeviceCSR:
    """Sorted CSR on the GPU: int32 rowptr/col, optional fp32 val, optional perm to the input order."""
    n_rows: int
    n_cols: int
    rowptr: Tensor
    col: Tensor
    val: Optional[Tensor] = None
    perm: Optional[Tensor] = None
    plan: Optional[SpmmPlan] = None
    hot: Optional[Tuple[int, int]] = None   # (first row, rows) of X worth an LDS cache in dense launches: see spmm()
    plan_bf16: Optional[SpmmPlan] = None    # spmm_bf16's own work-item plan: `plan` and the f32 launches are untouched by it
    plan_tiles: object = None               # the TILES plan of the dense launches (HUB_TILES): None = not tried, False = not applicable;
                                            # x_map / row_list launches keep `plan`
    hub_counts: dict = field(default_factory=dict)   # (hub_threshold, chunk) -> (hub rows, hub chunks): als_hub_counts

    # Value generation: 0 for an adjacency whose `val` is the one it was built with, a process-wide fresh number after every
    # later assignment of `val` and every invalidate_values().  With the identity and _version of the tensor itself it is
    # what a plan's value copies are checked against (_sync_plan_values).
    _val_gen = 0

    def __setattr__(self, name, value):
        if name == "val" and "val" in self.__dict__:
            object.__setattr__(self, "_val_gen", next(_VAL_GEN))
        object.__setattr__(self, name, value)

    def invalidate_values(self) -> None:
        """Tell the adjacency that the CONTENT of `val` was changed by a writer torch does not see: a kernel or a C-ABI
        caller given val.data_ptr(), a write through another tensor that aliases its storage.  The next spmm(self, ...)
        refreshes the value copies its plan holds.  Not needed after `self.val = tensor` or an in-place torch op on
        `self.val` itself: those are seen."""
        object.__setattr__(self, "_val_gen", next(_VAL_GEN))

    @property
    def nnz(self) -> int:
        return int(self.col.numel())

    @property
    def device(self):
        return self.rowptr.device


def coo_to_csr(row: Tensor, col: Tensor, n_rows: int, n_cols: int, want_perm: bool = True) -> DeviceCSR:
    """K4 — replaces SparseTensor(row=, col=, sparse_sizes=) (data/lightgcn_loader.py:65-79)."""
    _need(row, t.int64, "row")
    _need(col, t.int64, "col")
    if row.shape != col.shape or row.dim() != 1:
        raise ValueError("row/col must be 1-D tensors of equal length")
    nnz = row.numel()
    dev = row.device
    rowptr = t.empty(n_rows + 1, dtype=t.int32, device=dev)
    col_out = t.empty(nnz, dtype=t.int32, device=dev)
    perm = t.empty(nnz, dtype=t.int32, device=dev) if want_perm else None
    L = _lib.lib()
    ws = _ws(L.mi_coo_to_csr_workspace_bytes(n_rows, nnz), dev)
    check(L.mi_coo_to_csr_i32(n_rows, n_cols, nnz, _ptr(row), _ptr(col), _ptr(rowptr), _ptr(col_out),
                              _ptr(perm), ws.data_ptr(), ws.numel(), _stream()), "mi_coo_to_csr_i32")
    return DeviceCSR(n_rows, n_cols, rowptr, col_out, None, perm)


def csr_transpose(a: DeviceCSR) -> DeviceCSR:
    """CSR(A) -> CSR(A^T); values follow through perm_t (replaces csr2csc of torch_sparse)."""
    dev = a.device
    rowptr_t = t.empty(a.n_cols + 1, dtype=t.int32, device=dev)
    col_t = t.empty(a.nnz, dtype=t.int32, device=dev)
    perm_t = t.empty(a.nnz, dtype=t.int32, device=dev)
    L = _lib.lib()
    ws = _ws(L.mi_csr_transpose_workspace_bytes(a.n_rows, a.nnz), dev)
    check(L.mi_csr_transpose_i32(a.n_rows, a.n_cols, a.nnz, _ptr(a.rowptr), _ptr(a.col), _ptr(rowptr_t),
                                 _ptr(col_t), _ptr(perm_t), ws.data_ptr(), ws.numel(), _stream()),
          "mi_csr_transpose_i32")
    val_t = gather_f32(a.val, perm_t) if a.val is not None else None
    return DeviceCSR(a.n_cols, a.n_rows, rowptr_t, col_t, val_t, perm_t)


def gather_f32(src: Tensor, idx: Tensor) -> Tensor:
    _need(src, t.float32, "src")
    _need(idx, t.int32, "idx")
    out = t.empty(idx.numel(), dtype=t.float32, device=src.device)
    check(_lib.lib().mi_gather_f32(idx.numel(), _ptr(src), _ptr(idx), _ptr(out), _stream()), "mi_gather_f32")
    return out


def gcn_norm(a: DeviceCSR, val_in: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """K3 — gcn_norm(adj, add_self_loops=False) (model/lightgcn.py:56). Returns (val, deg^-1/2)."""
    if a.n_rows != a.n_cols:
        raise ValueError("gcn_norm needs a square adjacency")
    if val_in is not None:
        _need(val_in, t.float32, "val_in")
    val = t.empty(a.nnz, dtype=t.float32, device=a.device)
    dis = t.empty(a.n_rows, dtype=t.float32, device=a.device)
    check(_lib.lib().mi_gcn_norm_csr_f32(a.n_rows, a.nnz, _ptr(a.rowptr), _ptr(a.col), _ptr(val_in),
                                         _ptr(val), _ptr(dis), _stream()), "mi_gcn_norm_csr_f32")
    return val, dis


def scale_csr(a: DeviceCSR, val_in: Optional[Tensor] = None, row_scale: Optional[Tensor] = None,
              col_scale: Optional[Tensor] = None) -> Tensor:
    """val[p] = (val_in[p] * row_scale[row]) * col_scale[col]; None = ones."""
    for n, x in (("val_in", val_in), ("row_scale", row_scale), ("col_scale", col_scale)):
        if x is not None:
            _need(x, t.float32, n)
    if row_scale is not None and row_scale.numel() != a.n_rows:
        raise ValueError("row_scale must have one entry per row")
    if col_scale is not None and col_scale.numel() != a.n_cols:
        raise ValueError("col_scale must have one entry per column")
    out = t.empty(a.nnz, dtype=t.float32, device=a.device)
    check(_lib.lib().mi_scale_csr_f32(a.n_rows, a.nnz, _ptr(a.rowptr), _ptr(a.col), _ptr(val_in), _ptr(row_scale),
                                      _ptr(col_scale), _ptr(out), _stream()), "mi_scale_csr_f32")
    return out


def row_slice(a: DeviceCSR, r0: int, r1: int) -> DeviceCSR:
    """Rows [r0, r1) of `a` as a CSR that shares col/val storage (rowptr keeps absolute offsets)."""
    return DeviceCSR(r1 - r0, a.n_cols, a.rowptr[r0:r1 + 1], a.col, a.val, None, None, a.hot)


# LDS hot-row cache of the dense short-row launches (include/laplace_hip.h, mi_spmm_ex.hot_rows): module switches for A/B
# Persistent, software-pipelined short-row launch (+ optional LDS hot-row cache).  OFF by default: measured on C2 (round 3,
# profiles/r03_spmm_rows_persistent.md) it is 5-15 % SLOWER than the plain launch — the propagate runs at the chip's
# random-row gather ceiling for the bytes that miss L2 (5.0-5.5 TB/s of fabric traffic against the 5.5-5.8 TB/s the
# guide measures for random whole rows), rows the LDS cache serves were L2 hits already, and fewer resident wavefronts
# (86-105 VGPRs against 78) cost more than the shorter dependency chain returns.  Kept as a bitwise-equal alternative
# (tests/test_gpu_lightgcn.py) for graphs / parts whose balance differs.
PERSISTENT_ROWS = _os_environ.get("LAPLACE_PERSISTENT_ROWS", "0") == "1"
HOT_ROWS = int(_os_environ.get("LAPLACE_HOT_ROWS", 304))        # rows offered to the cache (the kernel clips to its LDS share); 0 = off
HOT_THREADS = int(_os_environ.get("LAPLACE_HOT_THREADS", 0))    # workgroup size of the persistent launch; 0 = the library's default


# Sliced short-row launch (include/laplace_hip.h, mi_spmm_ex.row_slices): 2 or 4 = the workgroups of an XCD compute one
# column slice of their rows, so the XCD's L2 holds that many times the gathered rows; 0 = the plain launch.  Applies to planned
# adjacencies that carry the `hot` hint (popularity-ordered items), for the rows in front of the hot rows (the user rows of a
# [users; items] adjacency; all rows where the hot rows start at 0).  Bitwise the plain launch; profiles/row_slices_c4.md.
# Measured on C4 (step, two streams): 2 slices gain 0.18 ms per plain dense launch and lose 0.36 ms with the Adam epilogue and
# 0.29 ms with x_map; 4 slices lose everywhere.  Hence the defaults: 2 slices, plain dense launches only.
ROW_SLICES = int(_os_environ.get("LAPLACE_SPMM_ROW_SLICES", 2))
ROW_SLICES_FORMS = int(_os_environ.get("LAPLACE_SPMM_ROW_SLICES_FORMS", 1))  # bit 0 plain dense launches, 1 Adam epilogue, 2 x_map
# Slices turn capacity misses into hits; where a column is gathered only a few times per pass most misses are first touches and
# the staging is pure cost.  Measured: C4 (1 000 gathers per item row and pass) gains 1.2 % per step, C2 (100) loses 2 %; nothing
# was measured in between, the bar sits between the two.
ROW_SLICES_MIN_REUSE = float(_os_environ.get("LAPLACE_SPMM_ROW_SLICES_MIN_REUSE", 400))


def _row_slices_pay(a: "DeviceCSR", plan: "SpmmPlan", slice_rows: int) -> bool:
    """Entries of the sliced rows per column they gather from >= ROW_SLICES_MIN_REUSE (one read-back per plan and hint)."""
    if ROW_SLICES_MIN_REUSE <= 0:
        return True
    if slice_rows not in plan.slice_reuse:
        nnz = int(a.rowptr[slice_rows]) if slice_rows else a.nnz
        cols = a.n_cols - (min(int(a.hot[0]), a.n_cols) if slice_rows else 0)
        plan.slice_reuse[slice_rows] = nnz / max(cols, 1)
    return plan.slice_reuse[slice_rows] >= ROW_SLICES_MIN_REUSE


def hot_item_rows(num_users: int, num_items: int) -> Optional[Tuple[int, int]]:
    """The `hot` hint of a [users; items] adjacency whose items are numbered by popularity (interactions.LocalityOrder):
    the first item rows are the ones most gathers go to."""
    if HOT_ROWS <= 0 or num_items <= 0:
        return None
    return (int(num_users), int(min(HOT_ROWS, num_items)))


SWEEP_BAND = 2048     # columns per band of a sweep plan: 2048 rows x 128 floats = 1 MB, a quarter of an XCD's L2
SWEEP_STREAMS = 1024  # sub-groups per XCD: 32 CUs x one workgroup of 32 sub-groups
SWEEP_MIN_BANDS = 64  # narrower adjacencies have nothing to sweep
SWEEP_PACE = 0        # pacing of the sweep: ticks (10 ns) per band of the time table; 0 = none


def build_sweep_plan(a: DeviceCSR, chunk: int = DEFAULT_CHUNK, band: int = SWEEP_BAND,
                     n_streams: int = SWEEP_STREAMS, min_deg: Optional[int] = None) -> Optional[SpmmPlan]:
    """SWEEP-form split-row plan (include/laplace_hip.h, mi_spmm_sweep), or None when the adjacency does not qualify
    (no long rows, fewer than SWEEP_MIN_BANDS bands, more row parts than the 8 * n_streams accumulators of an XCD,
    columns >= 2^28, no values yet).  Set-up: a few device sorts and one host pass over the long rows' degrees.
    min_deg (default: chunk): only the rows with MORE entries than this are laid out — the hub half of a hybrid plan
    (build_hybrid_plan), whose remaining split rows are banded work items."""
    import heapq
    if a.val is None or a.nnz == 0 or a.n_cols >= (1 << 27) or a.n_cols < SWEEP_MIN_BANDS * band:
        return None
    dev = a.device
    deg = (a.rowptr[1:] - a.rowptr[:-1]).to(t.int64)

    def slots_for(ch: int):
        rows = t.nonzero(deg > ch).view(-1)
        if rows.numel() == 0:
            return rows, [], 0, [], 0
        host = deg[rows].cpu().tolist()
        tot = sum(host)
        # parts per row: a slot should carry about a third of a stream's share, so that streams can be balanced
        target = max(ch, tot // (3 * n_streams))
        pp = [max(1, -(-d // target)) for d in host]
        return rows, host, tot, pp, sum(pp)

    long_rows, dl_host, total, parts, n_slots = slots_for(chunk if min_deg is None else max(int(min_deg), chunk))
    if long_rows.numel() == 0:
        return None
    if n_slots > 8 * n_streams:
        # More long rows than an XCD has accumulators (a graph whose typical row is long, e.g. C4's item rows).  Raising the
        # threshold until the longest rows fit was measured on C4 (round 2): dense launch 10.1 -> 10.7 ms against the banded
        # work items, so such adjacencies keep those.
        return None
    n_long = int(long_rows.numel())
    dl = deg[long_rows]
    # longest-processing-time assignment of slots to streams (<= 8 per stream)
    loads = []
    slot_base = [0] * (n_long + 1)
    for i, (d, p) in enumerate(zip(dl_host, parts)):
        slot_base[i + 1] = slot_base[i] + p
        loads += [(d / p, slot_base[i] + j) for j in range(p)]
    loads.sort(key=lambda z: (-z[0], z[1]))
    heap = [(0.0, k, 0) for k in range(n_streams)]
    heapq.heapify(heap)
    owner = [0] * n_slots
    qidx = [0] * n_slots
    slot_of = [-1] * (8 * n_streams)
    full = []
    for w, sid in loads:
        while True:
            load, k, cnt = heapq.heappop(heap)
            if cnt < 8:
                break
            full.append((load, k, cnt))
        owner[sid], qidx[sid] = k, cnt
        slot_of[k * 8 + cnt] = sid
        heapq.heappush(heap, (load + w, k, cnt + 1))
    owner_t = t.tensor(owner, dtype=t.int64, device=dev)
    q_t = t.tensor(qidx, dtype=t.int64, device=dev)
    parts_t = t.tensor(parts, dtype=t.int64, device=dev)
    base_t = t.tensor(slot_base, dtype=t.int64, device=dev)
    # entries of the long rows, in CSR order
    starts = a.rowptr[long_rows].to(t.int64)
    row_i = t.repeat_interleave(t.arange(n_long, device=dev), dl)                       # long-row index per entry
    first = t.cumsum(dl, 0) - dl
    e = starts[row_i] + (t.arange(total, device=dev) - first[row_i])                    # position in a.col / a.val
    c = a.col[e].to(t.int64)
    b = c // band
    n_b = (a.n_cols + band - 1) // band
    grp = row_i * n_b + b                                                               # (row, band): contiguous runs
    _, counts = t.unique_consecutive(grp, return_counts=True)
    g_first = t.cumsum(counts, 0) - counts
    g_of = t.repeat_interleave(t.arange(counts.numel(), device=dev), counts)
    rank = t.arange(total, device=dev) - g_first[g_of]
    part = (rank * parts_t[row_i]) // counts[g_of]                                      # equal consecutive pieces
    slot = base_t[row_i] + part
    x, tb = b & 7, b >> 3
    n_t = (n_b + 7) // 8
    key = (((x * n_streams + owner_t[slot]) * n_t + tb) << 3) | q_t[slot]
    order = t.argsort(key, stable=True)                                                 # columns stay ascending in a run
    skey = key[order]
    stream_key = (skey >> 3) // n_t
    band_key = skey >> 3                                                                # (stream, band)
    new_band = t.ones_like(band_key, dtype=t.bool)
    new_band[1:] = band_key[1:] != band_key[:-1]                                        # first entry of a band in its stream
    col_s = (((q_t[slot] << 28) | c)[order] | (new_band.to(t.int64) << 27)).to(t.int32).contiguous()
    src = e[order].to(t.int32).contiguous()                                             # kept: a re-weighting is one gather
    val_s = gather_f32(a.val, src)
    stream_ptr = t.searchsorted(stream_key, t.arange(8 * n_streams + 1, device=dev)).to(t.int32).contiguous()
    slot_of_t = t.tensor(slot_of, dtype=t.int32, device=dev)
    long_rows32 = long_rows.to(t.int32).contiguous()
    item_ptr = (8 * base_t).to(t.int32).contiguous()
    long_index = t.full((max(a.n_rows, 1),), -1, dtype=t.int32, device=dev)
    long_index[long_rows] = t.arange(n_long, dtype=t.int32, device=dev)
    st = SpmmPlanStruct()
    st.chunk, st.n_long_rows, st.n_items, st.n_launch = chunk, n_long, 8 * n_slots, 8 * n_slots
    st.long_rows, st.item_ptr, st.items = long_rows32.data_ptr(), item_ptr.data_ptr(), None
    st.long_index = long_index.data_ptr()
    st.band, st.n_bands = band, n_b
    # `epoch` carries the bands per XCD: read only by the MI_SWEEP_WG_SYNC experiment build of the kernel (profiles/r03_sweep.md)
    sw = SpmmSweepStruct(col_s.data_ptr(), val_s.data_ptr(), stream_ptr.data_ptr(), slot_of_t.data_ptr(), n_streams, n_slots,
                         None, int(n_t), max(SWEEP_PACE, 0))
    return SpmmPlan(st, long_rows32, item_ptr, None, long_index, sweep=sw, sweep_t=(col_s, val_s, stream_ptr, slot_of_t),
                    sweep_src=src, values_of=_values_key(a))


def sweep_degree_threshold(a: DeviceCSR, chunk: int, n_streams: int = SWEEP_STREAMS, fill: float = 1.0) -> Optional[int]:
    """The smallest degree T such that the rows with MORE than T entries fit the sweep form's 8 * n_streams row-part
    accumulators (build_sweep_plan's own part count: ceil(deg / max(chunk, total / (3 n_streams))) per row); None when even
    the single longest row does not, or no row is longer than chunk.  One host pass over the long rows' degrees."""
    import numpy as np
    deg = (a.rowptr[1:] - a.rowptr[:-1])
    dl = deg[deg > chunk]
    if dl.numel() == 0:
        return None
    ds = np.sort(dl.cpu().numpy().astype(np.int64))[::-1]           # descending
    cum = np.cumsum(ds)
    cap = int(8 * n_streams * fill)

    def slots(h):   # row parts of the h longest rows
        target = max(chunk, int(cum[h - 1]) // (3 * n_streams))
        return int(np.sum(-(-ds[:h] // target)))
    if slots(1) > cap:
        return None
    lo, hi = 1, len(ds)                                                # largest h with slots(h) <= cap (monotone in practice: checked)
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if slots(mid) <= cap:
            lo = mid
        else:
            hi = mid - 1
    h = lo
    if h == len(ds):
        return int(chunk)
    T = int(ds[h])                                                     # rows with deg > T: a prefix of the h longest (ties cut)
    while True:
        hh = int(np.searchsorted(-ds, -T, side="left"))                # number of rows with deg > T
        if hh == 0:
            return None
        if slots(hh) <= cap:
            return T
        T = int(ds[hh - 1])                                            # not monotone here: drop the shortest kept degree


def build_hybrid_plan(a: DeviceCSR, chunk: int = DEFAULT_CHUNK, band: Optional[int] = None, tail_whole: bool = False,
                      sweep_band: Optional[int] = None, n_streams: int = SWEEP_STREAMS) -> Optional[SpmmPlan]:
    """HYBRID split-row plan (round 4) for adjacencies whose typical row is long (C4's item rows: 100 K rows of ~10^3 entries):
    the hub rows — as many of the longest as the sweep form's 8 192 row-part accumulators hold, ~80 % of the entries on a
    Zipf graph — in SWEEP form (every row of X fetched into ONE XCD's L2 about once, 8 partial rows per row part), the
    remaining split rows either as banded work items (tail_whole=False) or, with the split threshold raised to the hub
    rows' degree, whole in the short-row kernel (tail_whole=True).  None when the adjacency does not qualify."""
    T = sweep_degree_threshold(a, chunk, n_streams)
    if T is None:
        return None
    sb = SWEEP_BAND if sweep_band is None else sweep_band
    if tail_whole or T <= chunk:
        return build_sweep_plan(a, chunk=max(T, chunk), band=sb, n_streams=n_streams)
    sw = build_sweep_plan(a, chunk=chunk, band=sb, n_streams=n_streams, min_deg=T)
    if sw is None:
        return None
    # the banded half: rows with chunk < degree <= T
    L = _lib.lib()
    if band is None:
        band = HYBRID_TAIL_BAND if a.n_cols >= MIN_BANDED_COLS else 0
    dev = a.device
    ws = _ws(L.mi_spmm_plan_workspace_bytes(a.n_rows, a.nnz), dev)
    info = _lib.SpmmPlanInfo()
    check(L.mi_spmm_plan_count_range(a.n_rows, a.n_cols, _ptr(a.rowptr), _ptr(a.col), chunk, T, band, ws.data_ptr(), ws.numel(),
                                     ctypes.byref(info), _stream()), "mi_spmm_plan_count_range")
    nl, nlaunch = int(info.n_long_rows), int(info.n_launch)
    if nl == 0:
        return sw
    long_rows_b = t.empty(nl, dtype=t.int32, device=dev)
    item_ptr_b = t.empty(nl + 1, dtype=t.int32, device=dev)
    items = t.empty(4 * max(nlaunch, 1), dtype=t.int32, device=dev)
    st_b = SpmmPlanStruct()
    st_b.long_rows, st_b.item_ptr, st_b.items, st_b.long_index = long_rows_b.data_ptr(), item_ptr_b.data_ptr(), items.data_ptr(), None
    check(L.mi_spmm_plan_fill(a.n_rows, _ptr(a.rowptr), ctypes.byref(info), ctypes.byref(st_b), ws.data_ptr(), ws.numel(),
                              _stream()), "mi_spmm_plan_fill")
    off = int(sw.struct.n_items)                                     # 8 * n_slots partial rows of the sweep come first
    it = items.view(-1, 4)
    it[:, 3] += (it[:, 3] >= 0).to(t.int32) * off                    # padding slots stay negative
    long_rows = t.cat([sw.long_rows, long_rows_b]).contiguous()
    item_ptr = t.cat([sw.item_ptr[:-1], item_ptr_b + off]).contiguous()
    long_index = t.full((max(a.n_rows, 1),), -1, dtype=t.int32, device=dev)
    long_index[long_rows.long()] = t.arange(long_rows.numel(), dtype=t.int32, device=dev)
    st = SpmmPlanStruct()
    st.chunk, st.n_long_rows = chunk, int(long_rows.numel())
    st.n_items, st.n_launch = off + int(info.n_items), nlaunch
    st.long_rows, st.item_ptr, st.items, st.long_index = long_rows.data_ptr(), item_ptr.data_ptr(), items.data_ptr(), long_index.data_ptr()
    st.band, st.n_bands = int(info.band), int(info.n_bands)
    return SpmmPlan(st, long_rows, item_ptr, items, long_index, sweep=sw.sweep, sweep_t=sw.sweep_t,
                    sweep_src=sw.sweep_src, values_of=sw.values_of)


HYBRID_TAIL_BAND = int(_os_environ.get("LAPLACE_HYBRID_TAIL_BAND", 16384))  # columns per band of a hybrid plan's banded tail


# HUB TILES (include/laplace_hip.h, mi_spmm_tiles; profiles/hub_tiles_c4.md): the longest split rows of an adjacency
# under the locality order are summed from LDS-staged tiles of X into register accumulators, every row of X read once per
# pass, instead of gathering through L2.  HUB_TILES: 0 = off, 1 = on for every dense launch of a planned adjacency with the
# `hot` hint that has hub rows (tests, A/B), "auto" = on where the gates below hold.  LAPLACE_SPMM_HUB_TILES overrides.
HUB_TILES = _os_environ.get("LAPLACE_SPMM_HUB_TILES", "auto")
HUB_SLOTS = int(_os_environ.get("LAPLACE_SPMM_HUB_SLOTS", 512))      # accumulators of a workgroup: 32 sub-groups x 16
HUB_FLOOR = int(_os_environ.get("LAPLACE_SPMM_HUB_FLOOR", 8192))     # hub rows have at least this many entries
HUB_TILE = int(_os_environ.get("LAPLACE_SPMM_HUB_TILE", 128))        # rows of X per tile: 64 or 128
# 1 = the kernel's streamed loads use the nt policy.  In-step A/B on C4, alternated three times: nt 46.09, 46.18, 45.80 ms per step,
# plain 45.79, 45.82, 45.30 (profiles/hub_tiles_c4.md, section 6): plain loads, bitwise the same result.
HUB_NT = int(_os_environ.get("LAPLACE_SPMM_HUB_NT", 0))
HUB_WGS = int(_os_environ.get("LAPLACE_SPMM_HUB_WGS", 0))            # workgroups (user ranges); 0 = the device's CU count
HUB_MIN_COLS = 1 << 20    # "auto": narrower operands sit in the L2s / the Infinity Cache and have nothing to stream for
# "auto": hub entries per streamed row of X.  A streamed row costs 512 B at D = 128; a hub entry's gather missed L2 for about
# 290 B on C4 (23.6 GB fetched for 81 M entries), so the stream pays from about 2 entries per row; the bar leaves a margin.
HUB_MIN_REUSE = float(_os_environ.get("LAPLACE_SPMM_HUB_MIN_REUSE", 4))
HUB_SG, HUB_ACC = 32, 16  # sub-groups per workgroup, accumulators per sub-group (csrc/spmm.hip, spmm_hub_tiles_kernel)
HUB_LOAD_COST = 6         # modelled cost of loading one row of a tile, in entries (user-range cuts): C4 averages 7 entries per row


def hub_tiles_slots(deg_desc, n_slots: int = 512, floor: int = 8192, n_sg: int = HUB_SG):
    """Which of the rows (degrees, longest first) become hub rows and into how many slots each is cut: (rows taken, parts per
    row, bound).  A row heavier than the mean load of a sub-group (bound = total hub entries // n_sg) is cut into
    k = ceil(deg / bound) classes — entry j of the row belongs to class j % k — so no slot is heavier than bound; rows are
    dropped from the short end until the slots fit n_slots.  Host arithmetic on at most n_slots numbers."""
    ds = [int(x) for x in deg_desc[:n_slots] if int(x) >= floor]
    while ds:
        bound = max(1, sum(ds) // n_sg)
        parts = [-(-x // bound) for x in ds]
        if sum(parts) <= n_slots:
            return len(ds), parts, bound
        ds.pop()
    return 0, [], 0


def hub_tiles_assign(loads, n_sg: int = HUB_SG, n_acc: int = HUB_ACC):
    """Longest-processing-time assignment of slots (entry counts) to sub-groups of n_acc accumulators: slot -> (sub-group,
    accumulator).  Ties by slot number: static."""
    import heapq
    order = sorted(range(len(loads)), key=lambda s: (-loads[s], s))
    heap = [(0, k, 0) for k in range(n_sg)]
    heapq.heapify(heap)
    where = [None] * len(loads)
    for s in order:
        while True:
            load, k, cnt = heapq.heappop(heap)
            if cnt < n_acc:
                break
        where[s] = (k, cnt)
        heapq.heappush(heap, (load + loads[s], k, cnt + 1))
    return where


def hub_tiles_ranges(tile_entries: Tensor, tile: int, n_wg: int) -> Tensor:
    """Cuts of the tiles into n_wg contiguous runs of about equal modelled cost: int64[n_wg + 1], tile numbers.  A tile
    without hub entries is never loaded and costs nothing; any other costs max(loading its rows, its entries)."""
    cost = t.where(tile_entries > 0, t.clamp(tile_entries, min=HUB_LOAD_COST * tile), t.zeros_like(tile_entries))
    cum = t.cumsum(cost, 0)
    total = int(cum[-1]) if cum.numel() else 0
    targets = (t.arange(1, n_wg, device=cum.device, dtype=t.int64) * total) // n_wg
    cuts = t.searchsorted(cum, targets, right=False) + 1   # the tile that crosses the target stays with the earlier workgroup
    z = t.zeros(1, dtype=t.int64, device=cum.device)
    return t.cat([z, t.clamp(cuts, max=cum.numel()), z + cum.numel()])


def build_hub_tiles_layout(a: DeviceCSR, hub_rows: Tensor, parts, n_wg: int, tile: int):
    """The tiles layout of the hub rows' entries (mi_spmm_tiles): a dict of tensors.  hub_rows: int64, parts[i] slots of row i.
    Torch ops on the adjacency's device (or the CPU, for the layout tests); set-up time only."""
    dev = a.rowptr.device
    n_hub = int(hub_rows.numel())
    deg = (a.rowptr[1:] - a.rowptr[:-1]).to(t.int64)
    dl = deg[hub_rows]
    total = int(dl.sum())
    parts_t = t.tensor(parts, dtype=t.int64, device=dev)
    base_t = t.cumsum(parts_t, 0) - parts_t
    n_slots = int(parts_t.sum())
    row_i = t.repeat_interleave(t.arange(n_hub, device=dev), dl)
    first = t.cumsum(dl, 0) - dl
    rank = t.arange(total, device=dev) - first[row_i]                                    # entry j of its row
    e = a.rowptr[hub_rows].to(t.int64)[row_i] + rank                                    # position in a.col / a.val
    c = a.col[e].to(t.int64)
    slot = base_t[row_i] + rank % parts_t[row_i]
    loads = t.bincount(slot, minlength=n_slots).cpu().tolist()
    where = hub_tiles_assign(loads)
    sg_t = t.tensor([w[0] for w in where], dtype=t.int64, device=dev)
    q_t = t.tensor([w[1] for w in where], dtype=t.int64, device=dev)
    slot_of = t.full((HUB_SG * HUB_ACC,), -1, dtype=t.int32, device=dev)
    slot_of[sg_t * HUB_ACC + q_t] = t.arange(n_slots, dtype=t.int32, device=dev)
    tl = c // tile
    n_tiles = (a.n_cols + tile - 1) // tile
    key = (tl * HUB_SG + sg_t[slot]) * HUB_ACC + q_t[slot]
    order = t.argsort(key, stable=True)                                                 # columns stay ascending within a slot
    key = key[order]
    tile_entries = t.bincount(tl, minlength=n_tiles)
    live = t.nonzero(tile_entries > 0).view(-1)                                         # the tiles that are loaded
    comp = t.full((n_tiles,), -1, dtype=t.int64, device=dev)
    comp[live] = t.arange(live.numel(), device=dev)
    n_live = int(live.numel())
    cnt = t.bincount(comp[key // (HUB_SG * HUB_ACC)] * (HUB_SG * HUB_ACC) + key % (HUB_SG * HUB_ACC),
                     minlength=n_live * HUB_SG * HUB_ACC).view(n_live, HUB_SG, HUB_ACC)
    per_sg = cnt.sum(2)
    sg_off = (t.cumsum(per_sg, 1) - per_sg).to(t.int32).contiguous()                   # first entry of the sub-group within its tile
    te = tile_entries[live]
    tile_ent = t.zeros(n_live + 1, dtype=t.int64, device=dev)
    tile_ent[1:] = t.cumsum(te, 0)
    cuts = hub_tiles_ranges(tile_entries, tile, n_wg)
    before = t.zeros(n_tiles + 1, dtype=t.int64, device=dev)
    before[1:] = t.cumsum((tile_entries > 0).to(t.int64), 0)
    src = e[order].to(t.int32).contiguous()
    return dict(ecol=(c[order] % tile).to(t.uint8).contiguous(), src=src, eval=a.val[src.long()].contiguous(),
                tile_id=live.to(t.int32).contiguous(), tile_ent=tile_ent.to(t.int32).contiguous(),
                cnt=cnt.to(t.uint8).contiguous(), sg_off=sg_off, wg_ptr=before[cuts].to(t.int32).contiguous(),
                wg_tiles=cuts, slot_of=slot_of, slot_loads=loads, n_slots=n_slots, item_ptr=(n_wg * t.cat([base_t, base_t.new_tensor([n_slots])])).to(t.int32).contiguous(),
                max_tile_entries=int(te.max()) if n_live else 0, tile=tile, n_wg=n_wg, cnt_max=int(cnt.max()) if n_live else 0)


def hub_tiles_entry_cap(tile: int, d: int = 128) -> int:
    """Entries of one tile that the kernel's LDS holds (csrc/spmm.hip: 3 entries staged per thread)."""
    lpr = 8 if d <= 32 else 16 if d <= 64 else 32
    return 3 * HUB_SG * lpr


def build_hub_tiles_plan(a: DeviceCSR, chunk: int = DEFAULT_CHUNK, n_slots: Optional[int] = None, floor: Optional[int] = None,
                         n_wg: Optional[int] = None, tile: Optional[int] = None) -> Optional[SpmmPlan]:
    """TILES plan: the hub rows (hub_tiles_slots) in the tiles layout, their n_wg partial rows per slot in front of the work
    items' slots; every other row as in build_spmm_plan's banded default (thin rows, banded work items up to the hub rows'
    degree), long_rows / item_ptr merged as the hybrid plan merges them.  None when the adjacency has no hub rows or a tile
    holds more entries than the kernel stages."""
    n_slots = HUB_SLOTS if n_slots is None else n_slots
    floor = HUB_FLOOR if floor is None else floor
    tile = HUB_TILE if tile is None else tile
    if n_wg is None:
        n_wg = HUB_WGS or t.cuda.get_device_properties(a.device).multi_processor_count
    if a.val is None or a.nnz == 0 or tile not in (64, 128) or not 0 < n_slots <= HUB_SG * HUB_ACC or n_wg < 1:
        return None
    dev = a.device
    deg = a.rowptr[1:] - a.rowptr[:-1]
    floor = max(floor, chunk + 1)
    cand = t.nonzero(deg >= floor).view(-1)
    if cand.numel() == 0:
        return None
    cand = cand[t.argsort(deg[cand], descending=True, stable=True)][:n_slots]
    n_hub, parts, _ = hub_tiles_slots(deg[cand].cpu().tolist(), n_slots, floor)
    if n_hub == 0:
        return None
    cand = cand[:n_hub]
    max_deg = int(deg[cand[-1]]) - 1                     # every row longer than this is a hub row ...
    hub_rows = t.nonzero(deg > max_deg).view(-1)         # ... ties of the shortest included
    if hub_rows.numel() != n_hub:
        hub_rows = hub_rows[t.argsort(deg[hub_rows], descending=True, stable=True)]
        n_hub, parts, _ = hub_tiles_slots(deg[hub_rows].cpu().tolist(), HUB_SG * HUB_ACC, floor)
        if n_hub != hub_rows.numel():
            return None                                  # a tie that does not fit: leave the adjacency to the banded plan
    else:
        hub_rows = cand
    lay = build_hub_tiles_layout(a, hub_rows.to(t.int64), parts, n_wg, tile)
    if lay["cnt_max"] > 255:                                      # duplicate entries beyond what a count byte holds
        return None
    if lay["max_tile_entries"] > hub_tiles_entry_cap(tile, 128):  # narrower products have smaller workgroups: checked per launch
        return None
    tl = _lib.SpmmTilesStruct(lay["ecol"].data_ptr(), lay["eval"].data_ptr(), lay["tile_id"].data_ptr(), lay["tile_ent"].data_ptr(),
                              lay["cnt"].data_ptr(), lay["sg_off"].data_ptr(), lay["wg_ptr"].data_ptr(), lay["slot_of"].data_ptr(),
                              n_wg, lay["n_slots"], tile, HUB_NT, a.n_cols, lay["max_tile_entries"])
    off = n_wg * lay["n_slots"]                           # the hub rows' partial rows come first
    hub32 = hub_rows.to(t.int32).contiguous()
    # the rest: thin rows and banded work items of the rows with chunk < degree <= max_deg
    L = _lib.lib()
    band = DEFAULT_BAND if a.n_cols >= MIN_BANDED_COLS else 0
    thin_max = THIN_PER_BAND * ((a.n_cols + band - 1) // band) if band > 0 else 0
    if thin_max <= chunk or thin_max > max_deg:
        thin_max = 0
    st = SpmmPlanStruct()
    plan = None
    nl = 0
    if max_deg > chunk:
        ws = _ws(L.mi_spmm_plan_workspace_bytes(a.n_rows, a.nnz), dev)
        info = _lib.SpmmPlanInfo()
        check(L.mi_spmm_plan_count_thin(a.n_rows, a.n_cols, _ptr(a.rowptr), _ptr(a.col), chunk, thin_max, max_deg, band,
                                        ws.data_ptr(), ws.numel(), ctypes.byref(info), _stream()), "mi_spmm_plan_count_thin")
        nl, nlaunch = int(info.n_long_rows), int(info.n_launch)
    long_index = t.full((max(a.n_rows, 1),), -1, dtype=t.int32, device=dev)
    if nl > 0:
        long_rows_b = t.empty(nl, dtype=t.int32, device=dev)
        item_ptr_b = t.empty(nl + 1, dtype=t.int32, device=dev)
        items = t.empty(4 * max(nlaunch, 1), dtype=t.int32, device=dev)
        st_b = SpmmPlanStruct()
        st_b.long_rows, st_b.item_ptr, st_b.items, st_b.long_index = long_rows_b.data_ptr(), item_ptr_b.data_ptr(), items.data_ptr(), None
        check(L.mi_spmm_plan_fill(a.n_rows, _ptr(a.rowptr), ctypes.byref(info), ctypes.byref(st_b), ws.data_ptr(), ws.numel(),
                                  _stream()), "mi_spmm_plan_fill")
        del ws
        it = items.view(-1, 4)
        it[:, 3] += (it[:, 3] >= 0).to(t.int32) * off    # padding slots stay negative
        long_rows = t.cat([hub32, long_rows_b]).contiguous()
        item_ptr = t.cat([lay["item_ptr"][:-1], item_ptr_b + off]).contiguous()
        st.n_items, st.n_launch = off + int(info.n_items), nlaunch
        st.items = items.data_ptr()
        st.band, st.n_bands = int(info.band), int(info.n_bands)
    else:
        items = None
        long_rows, item_ptr = hub32, lay["item_ptr"]
        st.n_items, st.n_launch = off, 0
        st.items = None
    long_index[long_rows.long()] = t.arange(long_rows.numel(), dtype=t.int32, device=dev)
    st.chunk, st.n_long_rows = chunk, int(long_rows.numel())
    st.long_rows, st.item_ptr, st.long_index = long_rows.data_ptr(), item_ptr.data_ptr(), long_index.data_ptr()
    plan = SpmmPlan(st, long_rows, item_ptr, items, long_index)
    plan.tiles, plan.tiles_t = tl, lay
    plan.thin_max = thin_max
    if thin_max > 0:
        rows = t.nonzero((deg > chunk) & (deg <= thin_max)).view(-1)
        if rows.numel() > 0:
            rows = rows[t.argsort(deg[rows], descending=True, stable=True)]
            long_index[rows] = -2
            plan.thin_rows = rows.to(t.int32).contiguous()
    if nl > 0:
        plan.nnz_long = int(info.nnz_long)
        if PACK_ENTRIES and nlaunch > 0 and plan.nnz_long > 0:
            # the work items' begin / end index the CSR arrays: the pack pass reads them as they are
            _pack_plan_entries(a, plan, values_only=False)
    plan.values_of = _values_key(a)
    return plan


def _hub_tiles_plan_for(a: DeviceCSR, d: int) -> Optional[SpmmPlan]:
    """The adjacency's tiles plan for a dense launch of width d, or None: the module switch, the gates of "auto", one build
    per adjacency (a.plan_tiles; False = tried and not applicable)."""
    if HUB_TILES in ("0", "", 0, None, False) or a.hot is None or d > 128 or d % 4:
        return None
    key = (str(HUB_TILES), HUB_SLOTS, HUB_FLOOR, HUB_TILE, HUB_NT, HUB_WGS, HUB_MIN_REUSE, id(a.plan))
    if a.__dict__.get("_plan_tiles_key") != key:      # another a.plan (rebuilt with another chunk) or other switches: build again
        object.__setattr__(a, "_plan_tiles_key", key)
        a.plan_tiles = None
    if a.plan_tiles is None:
        plan = None
        ok = a.nnz >= PLAN_MIN_NNZ or str(HUB_TILES) == "1"
        if ok and str(HUB_TILES) != "1":
            ok = a.n_cols >= HUB_MIN_COLS and a.plan is not None and a.plan.sweep is None
        if ok:
            plan = build_hub_tiles_plan(a, chunk=int(a.plan.struct.chunk) if a.plan is not None else DEFAULT_CHUNK)
        if plan is not None and str(HUB_TILES) != "1":
            if int(plan.tiles_t["tile_ent"][-1]) < HUB_MIN_REUSE * a.n_cols:
                plan = None
        a.plan_tiles = plan if plan is not None else False
    plan = a.plan_tiles or None
    if plan is not None and plan.tiles_t["max_tile_entries"] > hub_tiles_entry_cap(plan.tiles_t["tile"], d):
        return None                                       # this width's workgroup stages fewer entries per tile: today's path
    return plan


import os as _os
SWEEP = _os.environ.get("LAPLACE_SWEEP", "1") != "0"  # module switch (A/B): off keeps the banded work-item plans
SWEEP_BAND = int(_os.environ.get("LAPLACE_SWEEP_BAND", SWEEP_BAND))
SWEEP_PACE = int(_os.environ.get("LAPLACE_SWEEP_PACE", SWEEP_PACE))


def build_spmm_plan(a: DeviceCSR, chunk: int = DEFAULT_CHUNK, band: Optional[int] = None, sweep: Optional[bool] = None,
                    thin_max: Optional[int] = None) -> SpmmPlan:
    """Split-row plan of an adjacency.  band = columns per band of a banded plan (see include/laplace_hip.h),
    0 = row-major, None = DEFAULT_BAND when the adjacency has at least MIN_BANDED_COLS columns.  sweep (default: the
    module switch SWEEP, and only when band is not given): the SWEEP form when the adjacency qualifies.
    thin_max: rows with chunk < degree <= thin_max are THIN rows — no work items, no partial rows, summed whole by a
    wavefront each (plan.thin_rows, longest first); 0 = none.  None = 0 for every plan whose band is given, for sweep and
    row-major plans; THIN_PER_BAND * n_bands where the banded default applies."""
    if (SWEEP if sweep is None else sweep) and band is None:
        plan = build_sweep_plan(a, chunk, band=SWEEP_BAND)
        if plan is not None:
            return plan
    L = _lib.lib()
    if band is None:
        band = DEFAULT_BAND if a.n_cols >= MIN_BANDED_COLS else 0
        if thin_max is None and band > 0:
            thin_max = THIN_PER_BAND * ((a.n_cols + band - 1) // band)
    thin_max = int(thin_max or 0)
    if thin_max <= chunk:
        thin_max = 0
    dev = a.device
    ws = _ws(L.mi_spmm_plan_workspace_bytes(a.n_rows, a.nnz), dev)
    info = _lib.SpmmPlanInfo()
    check(L.mi_spmm_plan_count_thin(a.n_rows, a.n_cols, _ptr(a.rowptr), _ptr(a.col), chunk, thin_max, 2 ** 31 - 1, band,
                                    ws.data_ptr(), ws.numel(), ctypes.byref(info), _stream()), "mi_spmm_plan_count_thin")
    nl, nlaunch = int(info.n_long_rows), int(info.n_launch)
    long_rows = t.empty(max(nl, 1), dtype=t.int32, device=dev)
    item_ptr = t.empty(max(nl, 1) + 1, dtype=t.int32, device=dev)
    items = t.empty(4 * max(nlaunch, 1), dtype=t.int32, device=dev)
    long_index = t.empty(max(a.n_rows, 1), dtype=t.int32, device=dev)
    st = SpmmPlanStruct()
    st.long_rows, st.item_ptr, st.items = long_rows.data_ptr(), item_ptr.data_ptr(), items.data_ptr()
    st.long_index = long_index.data_ptr()
    check(L.mi_spmm_plan_fill(a.n_rows, _ptr(a.rowptr), ctypes.byref(info), ctypes.byref(st), ws.data_ptr(), ws.numel(),
                              _stream()), "mi_spmm_plan_fill")
    plan = SpmmPlan(st, long_rows, item_ptr, items, long_index)
    plan.nnz_long = int(info.nnz_long)
    del ws
    plan.thin_max = thin_max
    if thin_max > 0 and a.n_rows > 0:
        deg = a.rowptr[1:] - a.rowptr[:-1]
        rows = t.nonzero((deg > chunk) & (deg <= thin_max)).view(-1)
        if rows.numel() > 0:
            rows = rows[t.argsort(deg[rows], descending=True, stable=True)]
            long_index[rows] = -2                                   # row_list launches: "thin", neither short nor split
            plan.thin_rows = rows.to(t.int32).contiguous()
    if PACK_ENTRIES and nlaunch > 0 and plan.nnz_long > 0 and a.val is not None:
        _pack_plan_entries(a, plan, values_only=False)
        plan.values_of = _values_key(a)
    return plan


def _pack_plan_entries(a: DeviceCSR, plan: SpmmPlan, values_only: bool) -> None:
    """The split rows' (col, val) copied into launch order (mi_spmm_plan.epos / ecol / eval): a banded plan's work items are
    launched band by band, so in the CSR arrays every work item's ~12 entries sit in two cache lines of their own."""
    L = _lib.lib()
    dev, st = a.device, plan.struct
    if not values_only:
        plan.packed = (t.empty(int(st.n_launch), dtype=t.int32, device=dev), t.empty(plan.nnz_long, dtype=t.int32, device=dev),
                       t.empty(plan.nnz_long, dtype=t.float32, device=dev))
        st.epos, st.ecol, st.eval = (x.data_ptr() for x in plan.packed)
    ws = _ws(L.mi_spmm_plan_pack_workspace_bytes(int(st.n_launch)), dev)
    check(L.mi_spmm_plan_pack_entries(ctypes.byref(st), plan.nnz_long, _ptr(a.col), _ptr(a.val), 1 if values_only else 0,
                                      ws.data_ptr(), ws.numel(), _stream()), "mi_spmm_plan_pack_entries")


def _values_key(a: DeviceCSR) -> tuple:
    v = a.val
    return (v, v._version, a._val_gen)


def _sync_plan_values(a: DeviceCSR, plan: SpmmPlan) -> None:
    """Every value COPY a plan holds — packed[2] of a banded / row-major plan, val_s of a sweep or hybrid plan — follows
    a.val.  The plan remembers the tensor it copied from (a reference: its address cannot be handed to another tensor
    meanwhile, and an alias of equal data_ptr() and _version is another object), that tensor's _version (in-place torch
    ops) and the adjacency's value generation (DeviceCSR: assignment, invalidate_values()).  Unchanged = three
    comparisons on the host, no device work.  Changed = one pack pass / one gather into the EXISTING storage (the
    pointers inside the plan's structs stay), enqueued on the current stream ahead of the product."""
    v = a.val
    src, ver, gen = plan.values_of
    if src is v and ver == v._version and gen == a._val_gen:
        return
    _need(v, t.float32, "val")
    if v.numel() != a.nnz:
        raise ValueError(f"val has {v.numel()} entries, the adjacency {a.nnz}")
    if plan.packed:
        _pack_plan_entries(a, plan, values_only=True)
    if plan.tiles is not None:
        ev = plan.tiles_t["eval"]
        check(_lib.lib().mi_gather_f32(ev.numel(), _ptr(v), _ptr(plan.tiles_t["src"]), _ptr(ev), _stream()), "mi_gather_f32")
    if plan.sweep is not None:
        val_s = plan.sweep_t[1]
        check(_lib.lib().mi_gather_f32(val_s.numel(), _ptr(v), _ptr(plan.sweep_src), _ptr(val_s), _stream()), "mi_gather_f32")
    plan.values_of = _values_key(a)


def spmm(a: DeviceCSR, X: Tensor, *, Y: Optional[Tensor] = None, addend: Optional[Tensor] = None,
         S: Optional[Tensor] = None, scale: float = 1.0, x_map: Optional[Tensor] = None,
         addend_map: Optional[Tensor] = None, row_list: Optional[Tensor] = None,
         n_list_dev: Optional[Tensor] = None, adam: Optional[dict] = None, x_rare: bool = False) -> None:
    """K1/K2 — acc = A @ X; Y = acc (optional); S = scale * (addend + acc) (optional).

    adam = dict(p=, m=, v=, step=, lr=, beta1=, beta2=, eps=, reg_w=): S's value is the gradient of parameter
    table p and is consumed in registers by the Adam update (adam_step's arithmetic); S itself may be None.

    a.hot = (first row, rows): a speed hint for dense launches (no x_map / row_list) of a planned adjacency — those rows
    of X are cached in LDS by a persistent short-row launch.  Same values, same summation order: the result is bitwise
    the one without the hint.

    Sparse-operand forms (mi_spmm_csr_ex_f32): x_map int32[n_cols] — X is compact, column c reads
    X[x_map[c]], negative = an all-zero row; addend_map int32[n_rows] — addend is compact; row_list
    int32[n] (+ n_list_dev, device int32[1]) — compute only these rows, Y/S/addend compact by list position.
    x_rare (with x_map): few columns are live (mi_spmm_ex.x_bits) — the split rows' work items test a bitmap of the map
    first, gather only live entries and skip work items without any; bitwise the result without the hint.

    ROW_SLICES (module switch, 2 or 4) with a.hot set: the short rows of a planned launch run in the sliced form
    (mi_spmm_ex.row_slices) — a speed hint as well, bitwise the same result.

    Re-weighting: a plan holds copies of the split rows' values.  `a.val = tensor` and in-place torch ops on `a.val` are
    noticed by the next call (three integer / identity comparisons per call, _sync_plan_values); after a write torch cannot
    see — a kernel or C-ABI caller given a.val.data_ptr(), a write through an aliasing tensor — call a.invalidate_values()."""
    if a.val is None:
        raise ValueError("spmm needs edge values (run gcn_norm or set val)")
    d = X.shape[1]
    ldx = _rows_ok(X, "X")
    for nm, mp, ln in (("x_map", x_map, a.n_cols), ("addend_map", addend_map, a.n_rows)):
        if mp is not None:
            _need(mp, t.int32, nm)
            if mp.numel() != ln:
                raise ValueError(f"{nm} must have {ln} entries")
    if row_list is not None:
        _need(row_list, t.int32, "row_list")
        if addend_map is not None:
            raise ValueError("row_list and addend_map are exclusive (addend is indexed by list position)")
    if n_list_dev is not None:
        _need(n_list_dev, t.int32, "n_list_dev")
    if x_map is None and X.shape[0] != a.n_cols:
        raise ValueError(f"X has {X.shape[0]} rows, adjacency has {a.n_cols} columns")
    n_out = row_list.numel() if row_list is not None else a.n_rows
    for name, m in (("Y", Y), ("S", S)) + ((("addend", addend),) if addend_map is None else ()):
        if m is not None and (m.shape[0] != n_out or m.shape[1] != d):
            raise ValueError(f"{name} must be [{n_out}, {d}], got {tuple(m.shape)}")
    if addend is not None and addend.shape[1] != d:
        raise ValueError("addend width differs from X")
    if Y is None and S is None and adam is None:
        raise ValueError("spmm needs an output (Y and/or S)")
    if X.shape[0] == 0 and a.nnz == 0 and x_map is None and row_list is None and adam is None:
        # an adjacency without columns (a batch whose attribute relation holds no node): A @ X = 0, and X has no storage
        # to hand to the kernel
        if Y is not None:
            Y.zero_()
        if S is not None:
            S.copy_(addend * scale) if addend is not None else S.zero_()
        return
    adam_args = None
    if adam is not None:
        if row_list is not None:
            raise ValueError("the optimizer epilogue updates every parameter row: not with row_list")
        p_, m_, v_ = adam["p"], adam["m"], adam["v"]
        ldp = _rows_ok(p_, "adam.p")
        _need(m_, t.float32, "adam.m")
        _need(v_, t.float32, "adam.v")
        if tuple(p_.shape) != (a.n_rows, d) or m_.shape != p_.shape or v_.shape != p_.shape:
            raise ValueError(f"adam.p/m/v must be [{a.n_rows}, {d}]")
        rw = adam.get("reg_w")
        if rw is not None:
            _need(rw, t.float32, "adam.reg_w")
        adam_args = _lib.AdamArgs(p_.data_ptr(), ldp, m_.data_ptr(), v_.data_ptr(), _ptr(rw), float(adam["lr"]),
                                  float(adam.get("beta1", 0.9)), float(adam.get("beta2", 0.999)),
                                  float(adam.get("eps", 1e-8)), int(adam["step"]))
    ldy = _rows_ok(Y, "Y") if Y is not None else 0
    lda = _rows_ok(addend, "addend") if addend is not None else 0
    lds = _rows_ok(S, "S") if S is not None else 0
    if a.plan is None and (a.nnz >= PLAN_MIN_NNZ or row_list is not None):
        a.plan = build_spmm_plan(a)
    plan = a.plan
    if plan is not None and x_map is None and row_list is None:
        plan = _hub_tiles_plan_for(a, d) or plan          # dense launches: the hub rows from LDS-staged tiles (HUB_TILES)
    if plan is not None and plan.sweep is not None and d > 128:  # the sweep form stops at 128 floats per row
        if plan.wide is None:
            plan.wide = build_spmm_plan(a, chunk=int(plan.struct.chunk), sweep=False, thin_max=0)
        plan = plan.wide
    L = _lib.lib()
    if plan is not None and plan.values_of:
        _sync_plan_values(a, plan)                        # the adjacency was re-weighted since the plan copied its values?
    ws_ptr, ws_bytes = None, 0
    if plan is not None and plan.n_items > 0:
        if d not in plan.partial:
            plan.partial[d] = _ws(L.mi_spmm_workspace_bytes(ctypes.byref(plan.struct), d), a.device)
        ws_ptr, ws_bytes = plan.partial[d].data_ptr(), plan.partial[d].numel()
    col_ptr = _ptr(a.col) if a.nnz else a.rowptr.data_ptr()
    val_ptr = _ptr(a.val) if a.nnz else a.rowptr.data_ptr()
    ev = None
    if SPMM_EVENTS is not None:
        ev = (t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True))
        ev[0].record()
    sweep = plan.sweep if (plan is not None and plan.sweep is not None) else None
    hot_base, hot_rows = 0, (-1 if PERSISTENT_ROWS else 0)   # mi_spmm_ex.hot_rows: 0 = the plain launch, < 0 = persistent without a cache
    if (a.hot is not None and plan is not None and x_map is None and row_list is None and d <= 256 and HOT_ROWS > 0
            and PERSISTENT_ROWS):
        hot_base, hot_rows = int(a.hot[0]), int(a.hot[1])
        if hot_rows == 0:
            hot_rows = -1       # an empty range: still the persistent form the switch asks for
        if hot_base < 0 or hot_rows < -1 or hot_base + max(hot_rows, 0) > X.shape[0]:
            raise ValueError(f"hot rows [{hot_base}, {hot_base + hot_rows}) lie outside X ({X.shape[0]} rows)")

    x_bits = None
    if (x_rare and X_RARE_BITS and x_map is not None and row_list is None and sweep is None and plan is not None
            and plan.n_items > 0):
        x_bits = getattr(a, "_x_bits", None)
        if x_bits is None:
            x_bits = a._x_bits = t.empty((a.n_cols + 31) // 32, dtype=t.int32, device=a.device)
        check(L.mi_map_live_bits_i32(a.n_cols, _ptr(x_map), _ptr(x_bits), _stream()), "mi_map_live_bits_i32")

    n_thin = plan.n_thin_rows if plan is not None else 0
    form = 4 if x_map is not None else (2 if adam is not None else 1)
    row_slices = ROW_SLICES if (ROW_SLICES in (2, 4) and a.hot is not None and plan is not None and row_list is None
                                and (ROW_SLICES_FORMS & form)) else 0
    slice_rows = max(0, min(int(a.hot[0]), a.n_rows)) if row_slices else 0   # the rows in front of the hot rows: the user rows
    if row_slices and not _row_slices_pay(a, plan, slice_rows):
        row_slices = slice_rows = 0

    def launch(parts: int, stream: int, raw: bool = False):
        exs = None
        if (x_map is not None or addend_map is not None or row_list is not None or adam_args is not None or parts
                or sweep is not None or hot_rows != 0 or HOT_THREADS or n_thin or row_slices or (plan is not None and plan.tiles is not None)):
            exs = SpmmExStruct(_ptr(x_map), _ptr(addend_map), _ptr(row_list), _ptr(n_list_dev),
                               row_list.numel() if row_list is not None else 0,
                               ctypes.pointer(adam_args) if adam_args is not None else None, parts, hot_rows,
                               ctypes.pointer(sweep) if sweep is not None else None, hot_base, HOT_THREADS, _ptr(x_bits),
                               _ptr(plan.thin_rows) if n_thin else None, n_thin, row_slices, slice_rows,
                               ctypes.pointer(plan.tiles) if plan is not None and plan.tiles is not None else None)
        rc = L.mi_spmm_csr_ex_f32(a.n_rows, d, _ptr(a.rowptr), col_ptr, val_ptr, X.data_ptr(), ldx,
                                  _ptr(Y), ldy, _ptr(addend), lda, _ptr(S), lds, float(scale),
                                  ctypes.byref(plan.struct) if plan is not None else None,
                                  ctypes.byref(exs) if exs is not None else None, ws_ptr, ws_bytes, stream)
        if raw:
            return rc
        check(rc, "mi_spmm_csr_ex_f32")

    if plan is not None and plan.tiles is not None and d not in plan.tiles_t.setdefault("widths_ok", set()):
        # The first product of a tiles plan at this width is ONE whole launch on the current stream: the library tries the
        # tiles kernel's LDS size before it enqueues anything, so a device that refuses it (MI_ERR_UNSUPPORTED) has done no
        # work yet — the adjacency then gives up the form for good and the product is redone with its other plan.
        rc = launch(0, _stream(), raw=True)
        if rc == _lib.MI_ERR_UNSUPPORTED:
            a.plan_tiles = False
            return spmm(a, X, Y=Y, addend=addend, S=S, scale=scale, x_map=x_map, addend_map=addend_map, row_list=row_list,
                        n_list_dev=n_list_dev, adam=adam, x_rare=x_rare)
        check(rc, "mi_spmm_csr_ex_f32")
        plan.tiles_t["widths_ok"].add(d)
    elif SPMM_TWO_STREAMS and plan is not None and (plan.n_items > 0 or n_thin > 0):
        # short rows beside the split rows' work items + fix-up: disjoint output rows, joined before returning
        cur = t.cuda.current_stream()
        side = _side_stream(a.device)
        side.wait_stream(cur)
        if SPMM_TWO_STREAMS == 2:    # the split rows' one-workgroup-per-CU sweep takes its half of every CU first
            launch(_lib.MI_SPMM_SPLIT_ROWS, cur.cuda_stream)
            launch(_lib.MI_SPMM_SHORT_ROWS, side.cuda_stream)
        else:
            launch(_lib.MI_SPMM_SHORT_ROWS, side.cuda_stream)
            launch(_lib.MI_SPMM_SPLIT_ROWS, cur.cuda_stream)
        cur.wait_stream(side)
    else:
        launch(0, _stream())
    if ev is not None:
        ev[1].record()
        kind = "sparse" if (x_map is not None or row_list is not None) else ("dense_adam" if adam is not None else "dense")
        SPMM_EVENTS.append((ev[0], ev[1], kind, None, a.n_rows, a))


BF16_MAX_D = 256   # mi_spmm_csr_bf16: a row is at most 32 lanes of 8 elements


def check_bf16_width(d: int) -> None:
    """ValueError unless rows of d elements can be bf16 layer tables (mi_spmm_csr_bf16: d % 8 == 0, d <= 256)."""
    if d % 8 != 0:
        raise ValueError(f"bf16 layer tables need a width that is a multiple of 8 (16-byte row pieces), got d = {d}")
    if d > BF16_MAX_D:
        raise ValueError(f"bf16 layer tables stop at d = {BF16_MAX_D}, got d = {d}")


def _rows_ok_bf16(x: Tensor, name: str) -> int:
    """Checks a 2-D bf16 row-major matrix with unit inner stride; returns its leading dimension in elements."""
    _need(x, t.bfloat16, name, contiguous=False)
    if x.dim() != 2 or (x.shape[1] > 1 and x.stride(1) != 1):
        raise ValueError(f"{name}: expected a row-major 2-D matrix, got shape {tuple(x.shape)} strides {x.stride()}")
    return x.stride(0) if x.shape[0] > 1 else max(x.shape[1], x.stride(0))


def rows_to_bf16(src: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """The bf16 image of an f32 table, round to nearest even (mi_rows_f32_to_bf16); returns a torch.bfloat16 tensor."""
    lds_ = _rows_ok(src, "src")
    n, d = src.shape
    if out is None:
        out = t.empty(n, d, dtype=t.bfloat16, device=src.device)
    ldo = _rows_ok_bf16(out, "out")
    if tuple(out.shape) != (n, d):
        raise ValueError(f"out must be [{n}, {d}], got {tuple(out.shape)}")
    check(_lib.lib().mi_rows_f32_to_bf16(n, d, _ptr(src), lds_, _ptr(out), ldo, _stream()), "mi_rows_f32_to_bf16")
    return out


def spmm_bf16(a: DeviceCSR, X: Tensor, *, Y: Optional[Tensor] = None, addend: Optional[Tensor] = None,
              S: Optional[Tensor] = None, scale: float = 1.0, row_list: Optional[Tensor] = None,
              n_list_dev: Optional[Tensor] = None, plan: Optional[SpmmPlan] = None) -> None:
    """acc = A @ float(X) in f32 from a bf16 operand (mi_spmm_csr_bf16; the rule is in include/laplace_hip.h, "bf16 layer
    tables"): Y = rn(acc) in bf16 (optional); S = scale * (addend + (Y is given ? float(rn(acc)) : acc)) in f32 (optional).
    row_list int32[n] (+ n_list_dev, device int32[1]): only these rows, Y / S / addend compact by list position.

    plan=None uses a.plan_bf16, a slot of its own beside a.plan, built on first need under spmm's rule (nnz >= PLAN_MIN_NNZ
    or a row list) as build_spmm_plan(a, sweep=False, thin_max=0): work items only, since this product has neither the sweep
    form nor thin rows.  The f32 plan and its launches are untouched.  An explicit plan= (a work-item plan) overrides it.

    SPMM_TWO_STREAMS: the short rows run on the side stream beside the work items and the fix-up, as in spmm; equal bits
    either way.

    Re-weighting: val is read from the CSR arrays for every entry (a packed plan's copies are not used), so a re-weighted
    adjacency needs no _sync_plan_values here."""
    if a.val is None:
        raise ValueError("spmm_bf16 needs edge values (run gcn_norm or set val)")
    _need(a.val, t.float32, "val")
    ldx = _rows_ok_bf16(X, "X")
    d = X.shape[1]
    check_bf16_width(d)
    if X.shape[0] != a.n_cols:
        raise ValueError(f"X has {X.shape[0]} rows, adjacency has {a.n_cols} columns")
    if row_list is not None:
        _need(row_list, t.int32, "row_list")
    if n_list_dev is not None:
        _need(n_list_dev, t.int32, "n_list_dev")
        if row_list is None:
            raise ValueError("n_list_dev counts a row_list")
    n_out = row_list.numel() if row_list is not None else a.n_rows
    for name, m in (("Y", Y), ("S", S), ("addend", addend)):
        if m is not None and (m.dim() != 2 or m.shape[0] != n_out or m.shape[1] != d):
            raise ValueError(f"{name} must be [{n_out}, {d}], got {tuple(m.shape)}")
    if Y is None and S is None:
        raise ValueError("spmm_bf16 needs an output (Y and/or S)")
    ldy = _rows_ok_bf16(Y, "Y") if Y is not None else 0
    lda = _rows_ok(addend, "addend") if addend is not None else 0
    lds = _rows_ok(S, "S") if S is not None else 0
    if a.n_rows == 0 or n_out == 0:
        return
    if plan is None:
        if a.plan_bf16 is None and (a.nnz >= PLAN_MIN_NNZ or row_list is not None):
            a.plan_bf16 = build_spmm_plan(a, sweep=False, thin_max=0)
            st = a.plan_bf16.struct   # the packed (col, val) copies are never read here: give their memory back
            st.epos = st.ecol = st.eval = None
            a.plan_bf16.packed, a.plan_bf16.values_of = (), ()
        plan = a.plan_bf16
    if plan is not None and (plan.sweep is not None or plan.n_thin_rows):
        raise ValueError("spmm_bf16 takes a work-item plan: no sweep form, no thin rows")
    L = _lib.lib()
    ws_ptr, ws_bytes = None, 0
    if plan is not None and plan.n_items > 0:
        if d not in plan.partial:
            plan.partial[d] = _ws(L.mi_spmm_workspace_bytes(ctypes.byref(plan.struct), d), a.device)
        ws_ptr, ws_bytes = plan.partial[d].data_ptr(), plan.partial[d].numel()
    col_ptr = _ptr(a.col) if a.nnz else a.rowptr.data_ptr()
    val_ptr = _ptr(a.val) if a.nnz else a.rowptr.data_ptr()

    def launch(parts: int, stream: int) -> None:
        check(L.mi_spmm_csr_bf16(a.n_rows, d, _ptr(a.rowptr), col_ptr, val_ptr, X.data_ptr(), ldx, _ptr(Y), ldy,
                                 _ptr(addend), lda, _ptr(S), lds, float(scale),
                                 ctypes.byref(plan.struct) if plan is not None else None, _ptr(row_list), _ptr(n_list_dev),
                                 n_out if row_list is not None else 0, parts, ws_ptr, ws_bytes, stream), "mi_spmm_csr_bf16")

    if SPMM_TWO_STREAMS and plan is not None and plan.n_items > 0:
        cur = t.cuda.current_stream()
        side = _side_stream(a.device)
        side.wait_stream(cur)
        launch(_lib.MI_SPMM_SHORT_ROWS, side.cuda_stream)
        launch(_lib.MI_SPMM_SPLIT_ROWS, cur.cuda_stream)
        cur.wait_stream(side)
    else:
        launch(0, _stream())


def expand_rows(a: DeviceCSR) -> Tensor:
    out = t.empty(a.nnz, dtype=t.int32, device=a.device)
    check(_lib.lib().mi_csr_expand_rows(a.n_rows, _ptr(a.rowptr), _ptr(out), a.nnz, _stream()),
          "mi_csr_expand_rows")
    return out


def check_n_neg(n_neg: int) -> int:
    if not isinstance(n_neg, int) or isinstance(n_neg, bool) or not 1 <= n_neg <= _lib.MI_RANK_MAX_NEG:
        raise ValueError(f"n_neg must be an integer in 1..{_lib.MI_RANK_MAX_NEG}, got {n_neg!r}")
    return n_neg


def rank_objective_code(objective: str) -> int:
    """The C constant of a ranking objective name (ValueError for anything else)."""
    if objective not in _lib.MI_RANK_OBJECTIVES:
        raise ValueError(f"objective must be one of {sorted(_lib.MI_RANK_OBJECTIVES)}, got {objective!r}")
    return _lib.MI_RANK_OBJECTIVES[objective]


@dataclass
class NegativeTable:
    """The proposal of the popularity-weighted negative sampler (include/laplace_hip.h, "Popularity-weighted negatives"):
    item i is drawn with probability q_i / total.  cum holds the uint32 running sums of q as an int32 tensor of the same
    bits (torch has no uint32 arithmetic; nothing here computes on it); logq[i] = log(max(q_i, 1) / total) in fp32."""
    cum: Tensor
    logq: Tensor
    total: int
    power: Optional[float]
    n_items: int


def negative_counts(item_degree, power: float):
    """The integer weights q of the header's rule from item degrees, on the host in float64 (set-up, not a hot path):
    w = deg ** power where deg > 0, q = max(1, floor(w / sum(w) * 2^31)) there and 0 elsewhere."""
    import numpy as np
    if isinstance(power, bool) or not isinstance(power, (int, float)) or not 0.0 <= float(power) <= 1.0:
        raise ValueError(f"power must be a number in [0, 1], got {power!r}")
    deg = item_degree.detach().cpu().numpy() if isinstance(item_degree, Tensor) else np.asarray(item_degree)
    if deg.ndim != 1 or deg.shape[0] < 1 or deg.shape[0] >= 2**31:
        raise ValueError("item_degree: one degree per item, 1 <= n_items < 2^31")
    deg = deg.astype(np.float64)
    if not np.all(np.isfinite(deg)) or (deg < 0).any():
        raise ValueError("item_degree: finite degrees >= 0 expected")
    has = deg > 0
    if not has.any():
        raise ValueError("item_degree: every item has degree 0, nothing to draw from")
    w = np.where(has, np.power(np.where(has, deg, 1.0), float(power)), 0.0)
    s = float(np.cumsum(w)[-1])   # the sum in index order (np.sum adds pairwise)
    return np.where(has, np.maximum(1.0, np.floor(w / s * 2.0 ** 31)), 0.0).astype(np.int64)


def negative_table_from_counts(q, device, power: Optional[float] = None) -> NegativeTable:
    """NegativeTable from given integer weights q [n_items] (all >= 0, 0 < sum < 2^32)."""
    import numpy as np
    q = q.detach().cpu().numpy() if isinstance(q, Tensor) else np.asarray(q)
    if q.ndim != 1 or q.shape[0] < 1 or q.shape[0] >= 2**31 or q.dtype.kind not in "iu":
        raise ValueError("q: a 1-D integer array, 1 <= n_items < 2^31")
    q = q.astype(np.int64)
    if (q < 0).any():
        raise ValueError("q: weights >= 0 expected")
    cum = np.cumsum(q)
    total = int(cum[-1])
    if total <= 0:
        raise ValueError("q: every weight is 0, nothing to draw from")
    if total >= 2**32:
        raise ValueError(f"q: total weight {total} does not fit 32 bits")
    logq = np.log(np.maximum(q, 1).astype(np.float64) / float(total)).astype(np.float32)
    return NegativeTable(cum=t.from_numpy(cum.astype(np.uint32).view(np.int32)).to(device),
                         logq=t.from_numpy(logq).to(device), total=total, power=power, n_items=int(q.shape[0]))


def negative_table(item_degree, power: float = 0.75, device=None) -> NegativeTable:
    """Negatives drawn ∝ degree ** power (0 = uniform over the items that have a degree, 1 = ∝ degree; 0.75 is the usual
    choice).  item_degree: degrees in the TRAINING interactions, in the id space the sampler's CSR uses.  device: where the
    table lives (default: item_degree's if it is a tensor, else "cuda")."""
    q = negative_counts(item_degree, power)
    if device is None:
        device = item_degree.device if isinstance(item_degree, Tensor) else "cuda"
    return negative_table_from_counts(q, device, power=float(power))


def sample_bpr_batch(r: DeviceCSR, row_of_edge: Tensor, batch: int, neg_range: int, seed: int, step: int,
                     quirk: bool = False, out: Optional[Tuple[Tensor, Tensor, Tensor]] = None,
                     edges_in_order: bool = False, no_self_loops: bool = False, n_neg: int = 1,
                     table: Optional[NegativeTable] = None) -> Tuple[Tensor, Tensor, Tensor]:
    """K9 — replaces sample_mini_batch (data/lightgcn_loader.py:95-112) on device.  quirk: the reference's key
    collision; no_self_loops: structured_negative_sampling(contains_neg_self_loops=False) — never negative id == user id.
    n_neg > 1: neg is [batch, n_neg], independent draws per slot whose column 0 is the n_neg = 1 result.
    table: negatives drawn from the table's proposal instead of uniformly (mi_sample_bpr_batch_pop); users and pos are
    the uniform sampler's at the same (seed, step).  neg_range must be the table's n_items; no quirk bits."""
    check_n_neg(n_neg)
    if table is not None:
        if not isinstance(table, NegativeTable):
            raise TypeError(f"table: expected a NegativeTable, got {type(table)}")
        if int(neg_range) != table.n_items:
            raise ValueError(f"neg_range {neg_range} differs from the table's n_items {table.n_items}")
        if quirk or no_self_loops:
            raise ValueError("a negative table does not combine with quirk / no_self_loops")
        if batch < 1:
            raise ValueError("batch must be positive")
    if r.nnz == 0:
        raise ValueError("cannot sample from an empty edge set")
    if neg_range <= 0:
        raise ValueError("neg_range must be positive")
    dev = r.device
    if out is None:
        out = (t.empty(batch, dtype=t.int64, device=dev), t.empty(batch, dtype=t.int64, device=dev),
               t.empty(batch if n_neg == 1 else (batch, n_neg), dtype=t.int64, device=dev))
    users, pos, neg = out
    quirks = (1 if quirk else 0) | (2 if no_self_loops else 0)
    if table is not None:
        _need(table.cum, t.int32, "table.cum")
        for n, x in (("users", users), ("pos", pos), ("neg", neg)):
            _need(x, t.int64, "out: " + n)
        if table.cum.numel() != table.n_items:
            raise ValueError("table: cum must hold n_items words")
        if users.numel() != batch or pos.numel() != batch or neg.numel() != batch * n_neg:
            raise ValueError("out: users [batch], pos [batch], neg [batch * n_neg] expected")
        check(_lib.lib().mi_sample_bpr_batch_pop(batch, n_neg, r.nnz, _ptr(r.rowptr), _ptr(r.col), _ptr(row_of_edge),
                                                 table.n_items, _ptr(table.cum), 1 if edges_in_order else 0,
                                                 int(seed) & (2**64 - 1), int(step) & (2**64 - 1), _ptr(users),
                                                 _ptr(pos), _ptr(neg), _stream()), "mi_sample_bpr_batch_pop")
    elif n_neg == 1:
        check(_lib.lib().mi_sample_bpr_batch(batch, r.nnz, _ptr(r.rowptr), _ptr(r.col), _ptr(row_of_edge),
                                             int(neg_range), quirks,
                                             1 if edges_in_order else 0,
                                             int(seed) & (2**64 - 1),
                                             int(step) & (2**64 - 1), _ptr(users), _ptr(pos), _ptr(neg),
                                             _stream()), "mi_sample_bpr_batch")
    else:
        if neg.numel() != batch * n_neg:
            raise ValueError("out: neg must hold batch * n_neg ids")
        check(_lib.lib().mi_sample_bpr_batch_ex(batch, n_neg, r.nnz, _ptr(r.rowptr), _ptr(r.col), _ptr(row_of_edge),
                                                int(neg_range), quirks, 1 if edges_in_order else 0,
                                                int(seed) & (2**64 - 1), int(step) & (2**64 - 1), _ptr(users),
                                                _ptr(pos), _ptr(neg), _stream()), "mi_sample_bpr_batch_ex")
    return users, pos, neg


def rank_loss_fwd_bwd(users: Tensor, pos: Tensor, neg: Tensor, final_emb: Tensor, e0: Tensor, n_users: int,
                      lambda_val: float, *, objective: str = "reference", g_final: Optional[Tensor] = None,
                      reg_w: Optional[Tensor] = None, g_scale: float = 1.0, reg_scale: float = 1.0,
                      loss_out: Optional[Tensor] = None, node_map: Optional[Tensor] = None,
                      logq: Optional[Tensor] = None, _bpr_entry: bool = False) -> Tensor:
    """a7+a8 — batch gather + loss forward and backward with a choice of objective ("reference", "bpr", "softmax") and
    neg [B] or [B, M], M <= 16; ("reference", M = 1) is bpr_loss (utils/metrics_lightgcn.py:9-45).
    logq (float32, one entry per item of e0, addressed by item id): the logQ correction of the sampled softmax —
    the logits become s - logq[item] (mi_rank_loss_fwd_bwd_lq_f32); "softmax" only, and with g_final or without reg_w.
    _bpr_entry: bpr_fwd_bwd's switch to the C entry of the same case, mi_bpr_fwd_bwd_f32."""
    code = rank_objective_code(objective)
    if logq is not None and objective != "softmax":
        raise ValueError(f"logq corrects the sampled softmax only, not objective={objective!r}")
    batch = users.numel()
    if pos.numel() != batch or neg.dim() not in (1, 2) or neg.shape[0] != batch:
        raise ValueError("users [B], pos [B], neg [B] or [B, M] expected")
    n_neg = check_n_neg(1 if neg.dim() == 1 else int(neg.shape[1]))
    for n, x in (("users", users), ("pos", pos), ("neg", neg)):
        _need(x, t.int64, n)
    d = final_emb.shape[1]
    ldf = _rows_ok(final_emb, "final_emb")
    lde = _rows_ok(e0, "e0")
    ldg = _rows_ok(g_final, "g_final") if g_final is not None else 0
    if reg_w is not None:
        _need(reg_w, t.float32, "reg_w")
    dev = final_emb.device
    if loss_out is None:
        loss_out = t.empty(1, dtype=t.float32, device=dev)
    L = _lib.lib()
    ws = _ws(L.mi_rank_loss_workspace_bytes(batch, n_neg), dev)
    if _bpr_entry:
        if (objective, n_neg, logq) != ("reference", 1, None):
            raise ValueError("bpr_fwd_bwd is the reference objective over one negative per slot")
        check(L.mi_bpr_fwd_bwd_f32(batch, d, n_users, _ptr(users), _ptr(pos), _ptr(neg), final_emb.data_ptr(), ldf,
                                   e0.data_ptr(), lde, float(lambda_val), float(g_scale), float(reg_scale),
                                   loss_out.data_ptr(), _ptr(g_final), ldg, _ptr(reg_w), _ptr(node_map), ws.data_ptr(),
                                   ws.numel(), _stream()), "mi_bpr_fwd_bwd_f32")
        return loss_out
    if logq is None:
        check(L.mi_rank_loss_fwd_bwd_f32(batch, n_neg, code, d, n_users, _ptr(users), _ptr(pos), _ptr(neg),
                                         final_emb.data_ptr(), ldf, e0.data_ptr(), lde, float(lambda_val), float(g_scale),
                                         float(reg_scale), loss_out.data_ptr(), _ptr(g_final), ldg, _ptr(reg_w),
                                         _ptr(node_map), ws.data_ptr(), ws.numel(), _stream()), "mi_rank_loss_fwd_bwd_f32")
        return loss_out
    _need(logq, t.float32, "logq")
    if logq.dim() != 1 or logq.numel() != e0.shape[0] - n_users:
        raise ValueError(f"logq: one entry per item expected ({e0.shape[0] - n_users}), got shape {tuple(logq.shape)}")
    if g_final is None and reg_w is not None:
        raise ValueError("logq: the loss-only form takes no reg_w (pass g_final, or leave reg_w out)")
    check(L.mi_rank_loss_fwd_bwd_lq_f32(batch, n_neg, code, d, n_users, _ptr(users), _ptr(pos), _ptr(neg),
                                        final_emb.data_ptr(), ldf, e0.data_ptr(), lde, float(lambda_val), float(g_scale),
                                        float(reg_scale), loss_out.data_ptr(), _ptr(g_final), ldg, _ptr(reg_w),
                                        _ptr(node_map), logq.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
          "mi_rank_loss_fwd_bwd_lq_f32")
    return loss_out


def bpr_fwd_bwd(users: Tensor, pos: Tensor, neg: Tensor, final_emb: Tensor, e0: Tensor, n_users: int,
                lambda_val: float, *, g_final: Optional[Tensor] = None, reg_w: Optional[Tensor] = None,
                g_scale: float = 1.0, reg_scale: float = 1.0, loss_out: Optional[Tensor] = None,
                node_map: Optional[Tensor] = None) -> Tensor:
    """rank_loss_fwd_bwd(objective="reference") over one negative per slot, through the reference's own C entry."""
    return rank_loss_fwd_bwd(users, pos, neg, final_emb, e0, n_users, lambda_val, g_final=g_final, reg_w=reg_w,
                             g_scale=g_scale, reg_scale=reg_scale, loss_out=loss_out, node_map=node_map, _bpr_entry=True)


INBATCH_MAX_D = 256   # kMaxD of csrc/inbatch.hip


def check_inbatch_group(group: int) -> int:
    if not isinstance(group, int) or isinstance(group, bool) or not 32 <= group <= 4096 or group % 32:
        raise ValueError(f"group must be an integer multiple of 32 in 32..4096, got {group!r}")
    return group


def inbatch_softmax_fwd_bwd(users: Tensor, pos: Tensor, final_emb: Tensor, e0: Tensor, n_users: int, lambda_val: float, *,
                            group: int = 1024, logq: Optional[Tensor] = None, g_final: Optional[Tensor] = None,
                            reg_w: Optional[Tensor] = None, g_scale: float = 1.0, reg_scale: float = 1.0,
                            loss_out: Optional[Tensor] = None, node_map: Optional[Tensor] = None) -> Tensor:
    """In-batch sampled softmax (include/laplace_hip.h, "In-batch sampled softmax"): the candidates of slot b are the
    positives of its group of `group` consecutive slots, minus those that name slot b's item or belong to slot b's user;
    logq (float32, one entry per item of e0, by item id) is subtracted from the logits.  Conventions of rank_loss_fwd_bwd;
    the loss-only form (no g_final) takes no reg_w."""
    check_inbatch_group(group)
    if final_emb.dim() != 2:
        raise ValueError("final_emb: a 2-D table expected")
    d = int(final_emb.shape[1])
    if d < 4 or d % 4 or d > INBATCH_MAX_D:
        raise ValueError(f"the in-batch softmax needs d % 4 == 0 and d <= {INBATCH_MAX_D}, got d = {d}")
    batch = users.numel()
    if batch < 1 or pos.numel() != batch:
        raise ValueError("users [B], pos [B] expected, B >= 1")
    if g_final is None and reg_w is not None:
        raise ValueError("the loss-only form takes no reg_w (pass g_final, or leave reg_w out)")
    for n, x in (("users", users), ("pos", pos)):
        _need(x, t.int64, n)
    ldf = _rows_ok(final_emb, "final_emb")
    lde = _rows_ok(e0, "e0")
    ldg = _rows_ok(g_final, "g_final") if g_final is not None else 0
    if reg_w is not None:
        _need(reg_w, t.float32, "reg_w")
    if logq is not None:
        _need(logq, t.float32, "logq")
        if logq.dim() != 1 or logq.numel() != e0.shape[0] - n_users:
            raise ValueError(f"logq: one entry per item expected ({e0.shape[0] - n_users}), got shape {tuple(logq.shape)}")
    dev = final_emb.device
    if loss_out is None:
        loss_out = t.empty(1, dtype=t.float32, device=dev)
    L = _lib.lib()
    ws = _ws(L.mi_inbatch_softmax_workspace_bytes(batch, d, group), dev)
    check(L.mi_inbatch_softmax_fwd_bwd_f32(batch, group, d, n_users, _ptr(users), _ptr(pos), final_emb.data_ptr(), ldf,
                                           e0.data_ptr(), lde, float(lambda_val), float(g_scale), float(reg_scale),
                                           loss_out.data_ptr(), _ptr(g_final), ldg, _ptr(reg_w), _ptr(node_map),
                                           _ptr(logq), ws.data_ptr(), ws.numel(), _stream()),
          "mi_inbatch_softmax_fwd_bwd_f32")
    return loss_out


def full_softmax_fwd_bwd(users: Tensor, pos: Tensor, final_emb: Tensor, e0: Tensor, n_users: int, lambda_val: float, *,
                         g_final: Optional[Tensor] = None, reg_w: Optional[Tensor] = None, g_scale: float = 1.0,
                         reg_scale: float = 1.0, loss_out: Optional[Tensor] = None) -> Tensor:
    """Exact softmax over the whole catalogue (include/laplace_hip.h, "Full-catalogue softmax"): the candidates of slot b
    are all n_items = final_emb.shape[0] - n_users item rows of final_emb, with no mask and no logq.  g_final (all zero on
    entry) comes back with every item row written and the user rows the batch names; there is no node_map.  Conventions of
    inbatch_softmax_fwd_bwd; the loss-only form (no g_final) takes no reg_w."""
    if final_emb.dim() != 2:
        raise ValueError("final_emb: a 2-D table expected")
    d = int(final_emb.shape[1])
    if d < 4 or d % 4 or d > INBATCH_MAX_D:
        raise ValueError(f"the full softmax needs d % 4 == 0 and d <= {INBATCH_MAX_D}, got d = {d}")
    batch = users.numel()
    if batch < 1 or pos.numel() != batch:
        raise ValueError("users [B], pos [B] expected, B >= 1")
    n_items = int(final_emb.shape[0]) - int(n_users)
    if n_users < 0 or n_items < 1:
        raise ValueError(f"final_emb: {n_users} user rows and at least one item row expected, got {final_emb.shape[0]} rows")
    if g_final is None and reg_w is not None:
        raise ValueError("the loss-only form takes no reg_w (pass g_final, or leave reg_w out)")
    for n, x in (("users", users), ("pos", pos)):
        _need(x, t.int64, n)
    ldf = _rows_ok(final_emb, "final_emb")
    lde = _rows_ok(e0, "e0")
    ldg = _rows_ok(g_final, "g_final") if g_final is not None else 0
    if g_final is not None and g_final.shape[0] < final_emb.shape[0]:
        raise ValueError(f"g_final: {final_emb.shape[0]} rows expected (every item row is written), got {g_final.shape[0]}")
    if reg_w is not None:
        _need(reg_w, t.float32, "reg_w")
        if reg_w.numel() < final_emb.shape[0]:
            raise ValueError(f"reg_w: {final_emb.shape[0]} entries expected, got {reg_w.numel()}")
    dev = final_emb.device
    if loss_out is None:
        loss_out = t.empty(1, dtype=t.float32, device=dev)
    L = _lib.lib()
    ws = _ws(L.mi_full_softmax_workspace_bytes(batch, d, n_items), dev)
    check(L.mi_full_softmax_fwd_bwd_f32(batch, d, n_users, n_items, _ptr(users), _ptr(pos), final_emb.data_ptr(), ldf,
                                        e0.data_ptr(), lde, float(lambda_val), float(g_scale), float(reg_scale),
                                        loss_out.data_ptr(), _ptr(g_final), ldg, _ptr(reg_w), ws.data_ptr(), ws.numel(),
                                        _stream()),
          "mi_full_softmax_fwd_bwd_f32")
    return loss_out


def check_contrastive(d: int, *, eps: float = 0.0, tau: float = 1.0, group: int = 32) -> None:
    """The limits of perturb_rows / contrastive_fwd_bwd, each refusal naming its argument."""
    if d < 4 or d % 4 or d > INBATCH_MAX_D:
        raise ValueError(f"the contrastive term needs d % 4 == 0 and d <= {INBATCH_MAX_D}, got d = {d}")
    if isinstance(eps, bool) or not isinstance(eps, (int, float)) or not 0.0 <= eps < math.inf:
        raise ValueError(f"eps must be a finite number >= 0, got {eps!r}")
    if isinstance(tau, bool) or not isinstance(tau, (int, float)) or not 0.0 < tau < math.inf:
        raise ValueError(f"tau must be a finite number > 0, got {tau!r}")
    check_inbatch_group(group)


def perturb_rows(x: Tensor, *, eps: float, layer: int, seed: int, step: int, row_ids: Optional[Tensor] = None,
                 addend: Optional[Tensor] = None, S: Optional[Tensor] = None, scale: float = 1.0) -> Tensor:
    """x[r, :] += eps * sign(x[r, :]) * n[r, :] in place, n the unit noise vector of (seed, step, layer, the row's original
    id = row_ids[r], or r) — include/laplace_hip.h, "Noise-view contrastive term".  With S also S = (addend + x) * scale in
    the same pass (addend None: zero; S may be addend itself)."""
    if x.dim() != 2:
        raise ValueError("x: a 2-D table expected")
    n, d = int(x.shape[0]), int(x.shape[1])
    check_contrastive(d, eps=eps)
    if isinstance(layer, bool) or not isinstance(layer, int) or layer < 0:
        raise ValueError(f"layer must be an integer >= 0, got {layer!r}")
    ldx = _rows_ok(x, "x")
    if addend is not None and S is None:
        raise ValueError("addend without S: the sum has nowhere to go")
    if row_ids is not None:
        _need(row_ids, t.int64, "row_ids")
        if row_ids.numel() != n:
            raise ValueError(f"row_ids: one id per row expected ({n}), got {row_ids.numel()}")
    lda = lds = 0
    for name, y in (("addend", addend), ("S", S)):
        if y is not None and tuple(y.shape) != (n, d):
            raise ValueError(f"{name}: shape {(n, d)} expected, got {tuple(y.shape)}")
    if addend is not None:
        lda = _rows_ok(addend, "addend")
    if S is not None:
        lds = _rows_ok(S, "S")
    check(_lib.lib().mi_perturb_rows_f32(n, d, x.data_ptr(), ldx, _ptr(row_ids), float(eps), layer,
                                         int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1), _ptr(addend), lda, _ptr(S),
                                         lds, float(scale), _stream()), "mi_perturb_rows_f32")
    return x


def contrastive_fwd_bwd(ids: Tensor, a: Tensor, b: Tensor, *, tau: float, group: int = 1024, g_a: Optional[Tensor] = None,
                        g_b: Optional[Tensor] = None, g_scale_a: float = 1.0, g_scale_b: float = 1.0,
                        loss_out: Optional[Tensor] = None) -> Tensor:
    """InfoNCE between the normalised rows a[ids] and b[ids] over groups of `group` consecutive slots (include/laplace_hip.h,
    "Noise-view contrastive term"): slot b's candidates are the b-rows of its group, minus other slots that name its own id.
    g_a / g_b: the call ADDS g_scale_a * dloss/da and g_scale_b * dloss/db to the rows `ids` names; both or neither (the
    loss-only form).  Returns the loss as a 1-element device tensor."""
    if a.dim() != 2 or b.dim() != 2 or a.shape[1] != b.shape[1]:
        raise ValueError("a, b: two 2-D tables of one width expected")
    d = int(a.shape[1])
    check_contrastive(d, tau=tau, group=group)
    batch = ids.numel()
    if batch < 1 or ids.dim() != 1:
        raise ValueError("ids [B] expected, B >= 1")
    if (g_a is None) != (g_b is None):
        raise ValueError("g_a and g_b: both, or neither for the loss-only form")
    _need(ids, t.int64, "ids")
    lda, ldb = _rows_ok(a, "a"), _rows_ok(b, "b")
    ldga = ldgb = 0
    if g_a is not None:
        ldga, ldgb = _rows_ok(g_a, "g_a"), _rows_ok(g_b, "g_b")
        if g_a.shape != a.shape or g_b.shape != b.shape:
            raise ValueError("g_a, g_b: the shapes of a and b expected")
    dev = a.device
    if loss_out is None:
        loss_out = t.empty(1, dtype=t.float32, device=dev)
    L = _lib.lib()
    ws = _ws(L.mi_contrastive_workspace_bytes(batch, d, group), dev)
    check(L.mi_contrastive_fwd_bwd_f32(batch, group, d, ids.data_ptr(), a.data_ptr(), lda, b.data_ptr(), ldb, 1.0 / float(tau),
                                       loss_out.data_ptr(), _ptr(g_a), ldga, float(g_scale_a), _ptr(g_b), ldgb,
                                       float(g_scale_b), ws.data_ptr(), ws.numel(), _stream()), "mi_contrastive_fwd_bwd_f32")
    return loss_out


def adam_step(p: Tensor, grad: Tensor, m: Tensor, v: Tensor, *, step: int, lr: float, beta1: float = 0.9,
              beta2: float = 0.999, eps: float = 1e-8, reg_w: Optional[Tensor] = None) -> None:
    """a9 — dense Adam (torch.optim.Adam semantics) in one pass."""
    ldp = _rows_ok(p, "p")
    ldg = _rows_ok(grad, "grad")
    _need(m, t.float32, "m")
    _need(v, t.float32, "v")
    if m.shape != p.shape or v.shape != p.shape or grad.shape != p.shape:
        raise ValueError("p, grad, m, v must have equal shapes")
    check(_lib.lib().mi_adam_dense_f32(p.shape[0], p.shape[1], p.data_ptr(), ldp, grad.data_ptr(), ldg,
                                       m.data_ptr(), v.data_ptr(), _ptr(reg_w), float(lr), float(beta1),
                                       float(beta2), float(eps), int(step), _stream()), "mi_adam_dense_f32")


def gemm(A: Tensor, B: Tensor, *, trans_a: bool = False, trans_b: bool = True, bias: Optional[Tensor] = None,
         out: Optional[Tensor] = None, accumulate: bool = False, relu: bool = False) -> Tensor:
    """K6 — C = act(op(A) @ op(B) + bias (+ C)) on the f32 MFMA.  Defaults give nn.Linear: A [m, k],
    B = weight [n, k] (trans_b).  trans_a: A is stored [k, m];  trans_b=False: B is stored [k, n]."""
    lda = _rows_ok(A, "A")
    ldb = _rows_ok(B, "B")
    m, k = (A.shape[1], A.shape[0]) if trans_a else (A.shape[0], A.shape[1])
    n, kb = (B.shape[0], B.shape[1]) if trans_b else (B.shape[1], B.shape[0])
    if k != kb:
        raise ValueError(f"inner dimensions differ: {k} vs {kb}")
    if bias is not None:
        _need(bias, t.float32, "bias")
        if bias.numel() != n:
            raise ValueError("bias must have n entries")
    if out is None:
        if accumulate:
            raise ValueError("accumulate needs an output tensor")
        out = t.empty(m, n, dtype=t.float32, device=A.device)
    ldc = _rows_ok(out, "out")
    if out.shape != (m, n):
        raise ValueError(f"out must be [{m}, {n}]")
    L = _lib.lib()
    ws_bytes = L.mi_gemm_workspace_bytes(m, n, k)
    ws = _ws_reused(ws_bytes, A.device) if ws_bytes else None
    check(L.mi_gemm_f32(1 if trans_a else 0, 1 if trans_b else 0, m, n, k, _ptr(A), lda, _ptr(B), ldb,
                        _ptr(bias), out.data_ptr(), ldc, 1 if accumulate else 0, 1 if relu else 0,
                        ws.data_ptr() if ws is not None else None, ws_bytes, _stream()), "mi_gemm_f32")
    return out


def gemm_problem(A: Tensor, B: Tensor, out: Tensor, *, trans_a: bool = False, trans_b: bool = True,
                 A2: Optional[Tensor] = None, B2: Optional[Tensor] = None, a_mask: Optional[Tensor] = None,
                 bias: Optional[Tensor] = None, accumulate: bool = False, relu: bool = False):
    """One problem of gemm_group: out = act(op(A) @ op(B) [+ op(A2) @ op(B2)] + bias (+ out)); a_mask: A is read as 0
    where a_mask <= 0 (same shape and strides as A).  Shapes as in gemm().  Returns (descriptor, tensors): the
    descriptor holds raw pointers, the tuple keeps their storage alive until the launch has been enqueued."""
    lda, ldb, ldc = _rows_ok(A, "A"), _rows_ok(B, "B"), _rows_ok(out, "out")
    m, k = (A.shape[1], A.shape[0]) if trans_a else (A.shape[0], A.shape[1])
    n, kb = (B.shape[0], B.shape[1]) if trans_b else (B.shape[1], B.shape[0])
    if k != kb or tuple(out.shape) != (m, n):
        raise ValueError(f"gemm problem shapes differ: A {tuple(A.shape)}, B {tuple(B.shape)}, out {tuple(out.shape)}")
    k2 = lda2 = ldb2 = 0
    if A2 is not None:
        lda2, ldb2 = _rows_ok(A2, "A2"), _rows_ok(B2, "B2")
        m2, k2 = (A2.shape[1], A2.shape[0]) if trans_a else (A2.shape[0], A2.shape[1])
        n2, kb2 = (B2.shape[0], B2.shape[1]) if trans_b else (B2.shape[1], B2.shape[0])
        if (m2, n2) != (m, n) or k2 != kb2:
            raise ValueError("second pair must share m, n")
    if a_mask is not None and (_rows_ok(a_mask, "a_mask") != lda or a_mask.shape != A.shape):
        raise ValueError("a_mask must have A's shape and leading dimension")
    return (_lib.GemmProblem(1 if trans_a else 0, 1 if trans_b else 0, m, n, k, A.data_ptr(), lda, B.data_ptr(), ldb,
                             k2, _ptr(A2), lda2, _ptr(B2), ldb2, _ptr(a_mask), _ptr(bias), out.data_ptr(), ldc,
                             1 if accumulate else 0, 1 if relu else 0), (A, B, out, A2, B2, a_mask, bias))


def gemm_group(problems) -> bool:
    """Runs a list of gemm_problem()s in one launch per 8 (+ one grouped split-K reduce).  Returns False — nothing
    launched for that call — when an operand is not float4-addressable: the caller then issues gemm()s."""
    n = len(problems)
    if n == 0:
        return True
    arr = (_lib.GemmProblem * n)(*[p[0] for p in problems])  # p[1] keeps the operands alive across the allocation below
    L = _lib.lib()
    ws_bytes = L.mi_gemm_group_workspace_bytes(arr, n)
    ws = _ws_reused(ws_bytes, t.cuda.current_device()) if ws_bytes else None
    rc = L.mi_gemm_group_f32(arr, n, ws.data_ptr() if ws is not None else None, ws_bytes, _stream())
    if rc == _lib.MI_ERR_UNSUPPORTED:
        return False
    check(rc, "mi_gemm_group_f32")
    return True


TOPK_WS_BYTES = 2 << 30  # score block per launch; queries are processed in chunks of this size.  A/B at 100 K items, 65 536 queries
                         # (tools/bench_topk.py --ws-gib): 1 GiB (2 048 queries per chunk): 10.02 M / 8.03 M users/s (k = 12 / 256),
                         # 2 GiB (4 096): 10.63 M / 8.60 M, 4 GiB (8 192): 10.29 M / 8.09 M, 8 GiB (20 480): 10.69 M / 8.14 M
TOPK_CHUNK_QUANTUM = 2048  # chunks are multiples of this when they can be: the bf16 prefilter kernel (csrc/topk_prefilter.hpp)
                           # keeps 256 queries per workgroup and deals the workgroups of an item slice to one XCD's 32 CUs —
                           # 2 048 / 4 096 queries fill the chip in one round (100 K items: 4 096 per chunk)
# (Two-stream chunking: slower for the f32 fused kernel — 3.50-3.55 M -> 2.95-3.02 M users/s at k = 12, its grid fills the chip
# in whole rounds and a second one beside it breaks the rounds of both — but a gain for the bf16 prefilter path, which is the
# default: see TOPK_STREAMS below.)


# streams the chunks of one topk_excl call alternate over (each with its own workspace).  A/B, 65 536 queries against 100 K items
# (tools/bench_topk.py --streams N): 1: 8.45 M / 6.17 M users/s (k = 12 / 256), 2: 8.87 M / 6.70 M, 3: 8.55 M / 6.65 M — one
# chunk's side kernels (split, sample scores, threshold, refine) run beside the other's prefilter kernel, which holds one
# wavefront per SIMD and 96 KB of LDS per CU.  (The same switch was slower for the f32 fused kernel, whose grid fills the chip
# in whole rounds of two workgroups per CU.)
TOPK_STREAMS = int(_os_environ.get("LAPLACE_TOPK_STREAMS", 2))
_TOPK_SIDE = {}


def _topk_side_streams(dev, n: int):
    key = (t.device(dev).index if t.device(dev).index is not None else t.cuda.current_device(), n)
    if key not in _TOPK_SIDE:
        _TOPK_SIDE[key] = [t.cuda.Stream(device=dev) for _ in range(n)]
    return _TOPK_SIDE[key]


def topk_excl(uid: Tensor, user_emb: Tensor, item_emb: Tensor, k: int, excl: Optional[DeviceCSR] = None,
              want_scores: bool = False):
    """K10 — for each query user uid[q]: the k best item ids by (score desc, id asc) among items not in
    excl row q (a CSR with one row per query position).  Returns ids [n_q, k] (-1 pads) and optionally scores."""
    _need(uid, t.int64, "uid")
    ldu = _rows_ok(user_emb, "user_emb")
    ldi = _rows_ok(item_emb, "item_emb")
    n_q, n_items, d = uid.numel(), item_emb.shape[0], item_emb.shape[1]
    if user_emb.shape[1] != d:
        raise ValueError("user and item embeddings differ in width")
    if excl is not None and excl.n_rows != n_q:
        raise ValueError("exclusion CSR needs one row per query")
    dev = item_emb.device
    out_idx = t.empty(n_q, k, dtype=t.int64, device=dev)
    out_sc = t.empty(n_q, k, dtype=t.float32, device=dev) if want_scores else None
    L = _lib.lib()
    chunk = max(1, min(n_q, TOPK_WS_BYTES // max(4 * n_items, 1)))
    if n_q > chunk >= TOPK_CHUNK_QUANTUM:
        chunk -= chunk % TOPK_CHUNK_QUANTUM
    n_chunks = (n_q + chunk - 1) // chunk
    lanes = TOPK_STREAMS if (TOPK_STREAMS > 1 and n_chunks > 1) else 1
    # transient footprint = lanes x workspace (~2.2 GiB each at the default chunk): fall back to one lane, then to smaller
    # chunks, when the device does not have that much free
    ws_bytes = int(L.mi_topk_workspace_bytes(chunk, n_items, k))
    free = t.cuda.mem_get_info(dev)[0] + t.cuda.memory_reserved(dev) - t.cuda.memory_allocated(dev)
    if lanes > 1 and lanes * ws_bytes > 0.8 * free:
        lanes = 1
    while ws_bytes > 0.8 * free and chunk > 256:
        chunk = max(256, chunk // 2)
        ws_bytes = int(L.mi_topk_workspace_bytes(chunk, n_items, k))
    wss = [_ws(ws_bytes, dev) for _ in range(lanes)]

    prepared = {}   # workspace -> the chunk size whose item-side tables it holds (MI_TOPK_ITEMS_PREPARED)

    def launch(q0: int, ws: Tensor):
        q1 = min(n_q, q0 + chunk)
        # rowptr keeps absolute offsets into excl.col, so a chunk is just a slice of rowptr
        ep = excl.rowptr[q0:q1 + 1] if excl is not None else None
        ei = excl.col if (excl is not None and excl.nnz) else None
        # from a workspace's second chunk of the same size on, the item side of the prefilter (sample rows, the bf16 split of the
        # item table, the largest item norm: ~40 us per chunk at 100 K items) is still in it: same table, same layout
        flags = _lib.MI_TOPK_ITEMS_PREPARED if prepared.get(id(ws)) == q1 - q0 else 0
        check(L.mi_topk_excl_ex_f32(q1 - q0, n_items, d, k, uid[q0:q1].data_ptr(), user_emb.data_ptr(), ldu,
                                    item_emb.data_ptr(), ldi, _ptr(ep), _ptr(ei),
                                    out_idx[q0:q1].data_ptr(), out_sc[q0:q1].data_ptr() if want_scores else None,
                                    ws.data_ptr(), ws.numel(), flags, _stream()), "mi_topk_excl_ex_f32")
        prepared[id(ws)] = q1 - q0

    if lanes == 1:
        for q0 in range(0, n_q, chunk):
            launch(q0, wss[0])
    else:
        # chunks alternate over `lanes` streams, each with its own workspace: one chunk's side kernels (split, sample scores,
        # threshold, refine: ~30 % of its time) run beside the other's prefilter kernel, which holds one wavefront per SIMD
        cur = t.cuda.current_stream()
        side = _topk_side_streams(dev, lanes)
        for st in side:
            st.wait_stream(cur)
        for i, q0 in enumerate(range(0, n_q, chunk)):
            with t.cuda.stream(side[i % lanes]):
                launch(q0, wss[i % lanes])
        for st, ws in zip(side, wss):
            cur.wait_stream(st)
            ws.record_stream(st)
        for x in (uid, user_emb, item_emb, out_idx, out_sc, excl.rowptr if excl is not None else None,
                  excl.col if excl is not None else None):
            if x is not None:
                for st in side:
                    x.record_stream(st)
    return (out_idx, out_sc) if want_scores else out_idx


def topk_path(user_emb: Tensor, item_emb: Tensor, k: int) -> int:
    """Which code path of K10 topk_excl takes for these tables and this k (_lib.MI_TOPK_PATH_*: materialised, one pass, fused,
    fused LDS-DMA, bf16 prefilter) — asked of the dispatcher's own decision function; host-only, nothing is enqueued.  The
    choice does not depend on the number of queries, so it holds for every chunk of a chunked call."""
    ldu = _rows_ok(user_emb, "user_emb")
    ldi = _rows_ok(item_emb, "item_emb")
    n_items, d = item_emb.shape
    if user_emb.shape[1] != d:
        raise ValueError("user and item embeddings differ in width")
    rc = int(_lib.lib().mi_topk_path(n_items, d, k, user_emb.data_ptr(), ldu, item_emb.data_ptr(), ldi))
    check(rc if rc < 0 else 0, "mi_topk_path")
    return rc


RANK_WS_BYTES = 2 << 30    # workspace per launch of rank_of_items (path M's score block: 4 n_items bytes per row; exclusion
                           # bitmap: n_items / 8 bytes per row); rows are processed in chunks that fit
RANK_MAX_ROWS = 1 << 20    # and never more than this many rows per launch (the entry's limit is 65 535 panels of 64)


def rank_of_items(uid: Tensor, target: Tensor, user_emb: Tensor, item_emb: Tensor, excl: Optional[DeviceCSR] = None,
                  want_scores: bool = False, want_n_excluded: bool = False, chunk: Optional[int] = None,
                  ws: Optional[Tensor] = None):
    """K10r — for each query row p: how many items beat target[p] for user uid[p] in top-K's order (score desc, id asc) among
    the items not in excl row p (a CSR with one row per query position, as topk_excl's).  rank int32 [n_q]: -1 when the target is
    excluded or outside [0, n_items).  For k <= 1024, target[p] stands in column c of topk_excl's row iff rank[p] == c < k.
    Returns rank, then (want_scores) the target's score float32 [n_q] and (want_n_excluded) the number of distinct in-range
    ids of each exclusion row, int32 [n_q].  chunk: rows per launch (default: what fits RANK_WS_BYTES); one stream.
    ws: a uint8 workspace of the caller's to run in (it is cleared per call as far as the call reads it); too small is an error."""
    _need(uid, t.int64, "uid")
    _need(target, t.int64, "target")
    ldu = _rows_ok(user_emb, "user_emb")
    ldi = _rows_ok(item_emb, "item_emb")
    n_q, n_items, d = uid.numel(), item_emb.shape[0], item_emb.shape[1]
    if user_emb.shape[1] != d:
        raise ValueError("user and item embeddings differ in width")
    if target.numel() != n_q:
        raise ValueError("one target per query row expected")
    if excl is not None and excl.n_rows != n_q:
        raise ValueError("exclusion CSR needs one row per query")
    if chunk is not None and chunk < 1:
        raise ValueError("chunk must be positive")
    dev = item_emb.device
    rank = t.empty(n_q, dtype=t.int32, device=dev)
    score = t.empty(n_q, dtype=t.float32, device=dev) if want_scores else None
    n_ex = t.empty(n_q, dtype=t.int32, device=dev) if want_n_excluded else None
    L = _lib.lib()
    if chunk is None:
        chunk = max(1, min(n_q, RANK_MAX_ROWS))
        while chunk > 64 and int(L.mi_rank_items_workspace_bytes(chunk, n_items)) > RANK_WS_BYTES:
            chunk = (chunk + 1) // 2
    chunk = max(1, min(chunk, n_q))
    if ws is None:
        ws = _ws(int(L.mi_rank_items_workspace_bytes(chunk, n_items)), dev)
    else:
        _need(ws, t.uint8, "ws")
    for q0 in range(0, n_q, chunk):
        q1 = min(n_q, q0 + chunk)
        # rowptr keeps absolute offsets into excl.col, so a chunk is just a slice of rowptr
        ep = excl.rowptr[q0:q1 + 1] if excl is not None else None
        ei = excl.col if (excl is not None and excl.nnz) else None
        check(L.mi_rank_items_f32(q1 - q0, n_items, d, uid[q0:q1].data_ptr(), target[q0:q1].data_ptr(), user_emb.data_ptr(), ldu,
                                  item_emb.data_ptr(), ldi, _ptr(ep), _ptr(ei), rank[q0:q1].data_ptr(),
                                  score[q0:q1].data_ptr() if want_scores else None,
                                  n_ex[q0:q1].data_ptr() if want_n_excluded else None,
                                  ws.data_ptr(), ws.numel(), _stream()), "mi_rank_items_f32")
    out = (rank,) + ((score,) if want_scores else ()) + ((n_ex,) if want_n_excluded else ())
    return out if len(out) > 1 else rank


def rank_path(user_emb: Tensor, item_emb: Tensor) -> int:
    """Which code path rank_of_items takes for these tables (_lib.MI_RANK_PATH_FUSED / _MATERIALISED) — asked of the
    dispatcher's own decision function; host-only, nothing is enqueued.  It depends on neither the rows nor the chunk."""
    ldu = _rows_ok(user_emb, "user_emb")
    ldi = _rows_ok(item_emb, "item_emb")
    n_items, d = item_emb.shape
    if user_emb.shape[1] != d:
        raise ValueError("user and item embeddings differ in width")
    rc = int(_lib.lib().mi_rank_path(n_items, d, user_emb.data_ptr(), ldu, item_emb.data_ptr(), ldi))
    check(rc if rc < 0 else 0, "mi_rank_path")
    return rc


def topk_prefilter_scores(uid: Optional[Tensor], user_emb: Tensor, item_emb: Tensor) -> Tuple[Tensor, Tensor]:
    """Diagnostic of the bf16x3 prefilter behind topk_excl (csrc/topk_prefilter.hpp): the approximate scores [n_q, n_items]
    it compares with its thresholds and the per-query bound eps it assumes for |approximate - exact fma chain|."""
    ldu = _rows_ok(user_emb, "user_emb")
    ldi = _rows_ok(item_emb, "item_emb")
    n_q = uid.numel() if uid is not None else user_emb.shape[0]
    n_items, d = item_emb.shape
    if uid is not None:
        _need(uid, t.int64, "uid")
    dev = item_emb.device
    sc = t.empty(n_q, n_items, dtype=t.float32, device=dev)
    eps = t.empty(n_q, dtype=t.float32, device=dev)
    L = _lib.lib()
    ws = _ws(L.mi_topk_prefilter_scores_workspace_bytes(n_q, n_items), dev)
    check(L.mi_topk_prefilter_scores_f32(n_q, n_items, d, _ptr(uid), user_emb.data_ptr(), ldu, item_emb.data_ptr(), ldi,
                                         sc.data_ptr(), eps.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
          "mi_topk_prefilter_scores_f32")
    return sc, eps


def recent_items(ui_ptr: Tensor, ui_idx: Tensor, n_recent: int) -> Tuple[Tensor, Tensor]:
    """N5 recent-items recommender — the last n_recent distinct items of every row of a user -> item CSR (the last 64 entries
    are looked at, the most recent occurrence of an item counts): (items int64 [n_recent, n_users], slot 0 the latest item,
    unused slots filled with it; n_slots int32 [n_users])."""
    _need(ui_ptr, t.int32, "ui_ptr")
    _need(ui_idx, t.int32, "ui_idx")
    n_users = ui_ptr.numel() - 1
    if n_users < 0:
        raise ValueError("ui_ptr needs n_users + 1 entries")
    items = t.empty(int(n_recent), n_users, dtype=t.int64, device=ui_ptr.device)
    n_slots = t.empty(n_users, dtype=t.int32, device=ui_ptr.device)
    check(_lib.lib().mi_recent_items(n_users, ui_ptr.data_ptr(), ui_idx.data_ptr() if ui_idx.numel() else ui_ptr.data_ptr(),
                                     int(n_recent), _ptr(items), _ptr(n_slots), _stream()), "mi_recent_items")
    return items, n_slots


def pool_recent(items: Tensor, n_slots: Tensor, w: Tensor, table: Tensor) -> Tensor:
    """N5 recent-items recommender, pool = "mean" — q[u] = (sum_r w[r] * table[items[r, u]]) / (sum_r w[r]) over the user's
    n_slots[u] slots, r ascending, every operation one float32 rounding.  Returns q float32 [n_users, d]."""
    _need(items, t.int64, "items")
    _need(n_slots, t.int32, "n_slots")
    _need(w, t.float32, "w")
    ld = _rows_ok(table, "table")
    if items.dim() != 2 or n_slots.numel() != items.shape[1] or w.numel() != items.shape[0]:
        raise ValueError("items must be [n_recent, n_users] with one n_slots entry per user and one weight per slot")
    n_recent, n_users = items.shape
    d = table.shape[1]
    q = t.empty(n_users, d, dtype=t.float32, device=table.device)
    check(_lib.lib().mi_pool_recent_f32(n_users, n_recent, d, _ptr(items), _ptr(n_slots), w.data_ptr(), table.data_ptr(), ld,
                                        _ptr(q), d, _stream()), "mi_pool_recent_f32")
    return q


def topk_merge_max(ids: Tensor, scores: Tensor, n_slots: Tensor, w: Tensor, k_out: int, want_scores: bool = True):
    """N5 recent-items recommender, pool = "max" — merges per-slot top-K lists (ids int64 / scores float32
    [n_lists, n_q, k_in], -1 pads): an item's score is the maximum of w[r] * score over its entries in the lists
    r < n_slots[q]; returns the k_out best by (score desc, id asc) as ids [n_q, k_out] (-1 pads) and optionally scores
    (-inf pads).  n_lists * k_in <= 4096, k_out <= k_in."""
    _need(ids, t.int64, "ids")
    _need(scores, t.float32, "scores")
    _need(n_slots, t.int32, "n_slots")
    _need(w, t.float32, "w")
    if ids.dim() != 3 or scores.shape != ids.shape or n_slots.numel() != ids.shape[1] or w.numel() != ids.shape[0]:
        raise ValueError("ids and scores must be [n_lists, n_q, k_in] with one n_slots entry per query and one weight per list")
    n_lists, n_q, k_in = ids.shape
    out_ids = t.empty(n_q, int(k_out), dtype=t.int64, device=ids.device)
    out_sc = t.empty(n_q, int(k_out), dtype=t.float32, device=ids.device) if want_scores else None
    check(_lib.lib().mi_topk_merge_max_f32(n_q, n_lists, k_in, int(k_out), _ptr(ids), _ptr(scores), _ptr(n_slots), w.data_ptr(),
                                           _ptr(out_ids), _ptr(out_sc), _stream()), "mi_topk_merge_max_f32")
    return (out_ids, out_sc) if want_scores else out_ids


def segment_max(a: DeviceCSR, X: Tensor, want_arg: bool = True):
    """K5 (aggr="max") — Y[r] = max over the sources of destination r (0 for none); arg = winning source ids."""
    ldx = _rows_ok(X, "X")
    d = X.shape[1]
    Y = t.empty(a.n_rows, d, dtype=t.float32, device=X.device)
    arg = t.empty(a.n_rows, d, dtype=t.int32, device=X.device) if want_arg else None
    colp = _ptr(a.col) if a.nnz else a.rowptr.data_ptr()
    check(_lib.lib().mi_segment_max_f32(a.n_rows, d, _ptr(a.rowptr), colp, X.data_ptr(), ldx, Y.data_ptr(), d,
                                        _ptr(arg), _stream()), "mi_segment_max_f32")
    return Y, arg


def segment_max_bwd(by_src: DeviceCSR, arg: Tensor, dY: Tensor) -> Tensor:
    """Gradient of segment_max wrt X: by_src is the same relation as a CSR over SOURCE nodes (col = destination ids).
    Deterministic: each dX element has one writer that sums its destinations in CSR order."""
    _need(arg, t.int32, "arg")
    ldy = _rows_ok(dY, "dY")
    d = dY.shape[1]
    dX = t.empty(by_src.n_rows, d, dtype=t.float32, device=dY.device)
    if by_src.n_rows:
        colp = _ptr(by_src.col) if by_src.nnz else by_src.rowptr.data_ptr()
        check(_lib.lib().mi_segment_max_bwd_f32(by_src.n_rows, d, _ptr(by_src.rowptr), colp, arg.data_ptr(),
                                                dY.data_ptr() if dY.numel() else None, ldy, dX.data_ptr(), d, _stream()),
              "mi_segment_max_bwd_f32")
    return dX


def embed_concat(x: Tensor, tables, max_norm: float = 1.0) -> Tensor:
    """K7 — cat_i Embedding_i(max_norm)(x[:, i]).  tables: list of [rows_i, dim_i] fp32 GPU tensors."""
    _need(x, t.int64, "x")
    if x.dim() != 2 or x.shape[1] != len(tables):
        raise ValueError("x must be [n, n_cols] with one table per column")
    for i, tb in enumerate(tables):
        _need(tb, t.float32, f"tables[{i}]")
    n, nc = x.shape
    width = sum(int(tb.shape[1]) for tb in tables)
    out = t.empty(n, width, dtype=t.float32, device=x.device)
    if n == 0 or nc == 0:
        return out
    off = 0
    for c0 in range(0, nc, 16):  # the kernel takes up to 16 table descriptors by value: wider inputs go in groups
        tabs = tables[c0:c0 + 16]
        g = len(tabs)
        xs = x if (c0 == 0 and g == nc) else x[:, c0:c0 + g].contiguous()
        ptrs = (ctypes.c_void_p * g)(*[tb.data_ptr() for tb in tabs])
        rows = (ctypes.c_int64 * g)(*[int(tb.shape[0]) for tb in tabs])
        dims = (ctypes.c_int32 * g)(*[int(tb.shape[1]) for tb in tabs])
        check(_lib.lib().mi_embed_concat_f32(n, g, xs.data_ptr(), ptrs, rows, dims, float(max_norm),
                                             out.data_ptr() + 4 * off, width, _stream()), "mi_embed_concat_f32")
        off += sum(int(tb.shape[1]) for tb in tabs)
    return out


def match_common_items(users_ptr: Tensor, users_idx: Tensor, articles_ptr: Tensor, articles_idx: Tensor, k: int,
                       query_users: Optional[Tensor] = None, n_queries: Optional[int] = None):
    """N3 — UsersWithCommonItemsMatcher for many users at once: (out int32[n, k] with -1 pads, counts int32[n])."""
    for n, x in (("users_ptr", users_ptr), ("users_idx", users_idx), ("articles_ptr", articles_ptr), ("articles_idx", articles_idx)):
        _need(x, t.int32, n)
    if query_users is not None:
        _need(query_users, t.int64, "query_users")
        n_queries = query_users.numel()
    elif n_queries is None:
        n_queries = users_ptr.numel() - 1
    out = t.empty(n_queries, int(k), dtype=t.int32, device=users_ptr.device)
    cnt = t.empty(n_queries, dtype=t.int32, device=users_ptr.device)
    check(_lib.lib().mi_match_common_items_i32(n_queries, _ptr(query_users), users_ptr.data_ptr(), users_idx.data_ptr() if users_idx.numel() else users_ptr.data_ptr(),
                                               articles_ptr.data_ptr(), articles_idx.data_ptr() if articles_idx.numel() else articles_ptr.data_ptr(),
                                               int(k), _ptr(out), _ptr(cnt), _stream()), "mi_match_common_items_i32")
    return out, cnt


def match_same_location(location_of_user: Tensor, loc_ptr: Tensor, loc_idx: Tensor, users_ptr: Tensor, users_idx: Tensor,
                        k: int, query_users: Optional[Tensor] = None, n_queries: Optional[int] = None):
    """N3 — UsersSameLocationMatcher for many users at once: (out int32[n, k] with -1 pads, counts int32[n])."""
    for n, x in (("location_of_user", location_of_user), ("loc_ptr", loc_ptr), ("loc_idx", loc_idx),
                 ("users_ptr", users_ptr), ("users_idx", users_idx)):
        _need(x, t.int32, n)
    if query_users is not None:
        _need(query_users, t.int64, "query_users")
        n_queries = query_users.numel()
    elif n_queries is None:
        n_queries = location_of_user.numel()
    if location_of_user.numel() != users_ptr.numel() - 1:
        raise ValueError("location_of_user must have one entry per user")
    dev = users_ptr.device
    out = t.empty(n_queries, int(k), dtype=t.int32, device=dev)
    cnt = t.empty(n_queries, dtype=t.int32, device=dev)
    check(_lib.lib().mi_match_same_location_i32(n_queries, _ptr(query_users), location_of_user.data_ptr(), loc_ptr.data_ptr(),
                                                loc_idx.data_ptr() if loc_idx.numel() else loc_ptr.data_ptr(),
                                                users_ptr.data_ptr(), users_idx.data_ptr() if users_idx.numel() else users_ptr.data_ptr(),
                                                int(k), _ptr(out), _ptr(cnt), _stream()), "mi_match_same_location_i32")
    return out, cnt


_COOC_WS = {}


def _cooc_ws(which: str, nbytes: int, device) -> Tensor:
    """One grow-only workspace per device and stage, sized by the library's own query."""
    key = (t.device(device).index, which)
    if key not in _COOC_WS or _COOC_WS[key].numel() < nbytes:
        _COOC_WS[key] = _ws(nbytes, device)
    return _COOC_WS[key]


def cooc_item_neighbors(users_ptr: Tensor, users_idx: Tensor, articles_ptr: Tensor, articles_idx: Tensor, T: int,
                        weighting: str = "cosine"):
    """N3b stage 1 — the item neighbour table of the co-occurrence matcher: (ids int32[I, T] with -1 pads, counts int32[I, T],
    scores float32[I, T]); row i = the T best j by c(i, j) = (A^T A)[i, j] ("count") or c / sqrt(d_i d_j) ("cosine")."""
    for n, x in (("users_ptr", users_ptr), ("users_idx", users_idx), ("articles_ptr", articles_ptr), ("articles_idx", articles_idx)):
        _need(x, t.int32, n)
    if weighting not in _lib.MI_COOC_WEIGHTINGS:
        raise ValueError(f"weighting: expected one of {sorted(_lib.MI_COOC_WEIGHTINGS)}, got {weighting!r}")
    if users_idx.numel() != articles_idx.numel():
        raise ValueError("users_idx and articles_idx must list the same edges")
    T = int(T)
    n_users, n_items, nnz, dev = users_ptr.numel() - 1, articles_ptr.numel() - 1, users_idx.numel(), users_ptr.device
    L = _lib.lib()
    need = L.mi_cooc_items_workspace_bytes(n_items, nnz, T)
    if need == 0:
        raise ValueError(f"cooc_item_neighbors: T = {T} outside 1..64, or sizes beyond int32 indexing")
    ws = _cooc_ws("items", need, dev)
    ids = t.empty(n_items, T, dtype=t.int32, device=dev)
    counts = t.empty(n_items, T, dtype=t.int32, device=dev)
    scores = t.empty(n_items, T, dtype=t.float32, device=dev)
    check(L.mi_cooc_items_topt(n_users, n_items, nnz, users_ptr.data_ptr(), _ptr(users_idx), articles_ptr.data_ptr(),
                               _ptr(articles_idx), T, _lib.MI_COOC_WEIGHTINGS[weighting], _ptr(ids), _ptr(counts), _ptr(scores),
                               ws.data_ptr(), ws.numel(), _stream()), "mi_cooc_items_topt")
    return ids, counts, scores


def match_cooccurrence(users_ptr: Tensor, users_idx: Tensor, nbr_id: Tensor, nbr_score: Tensor, k: int,
                       n_queries: Optional[int] = None, query_users: Optional[Tensor] = None, n_recent: Optional[int] = None,
                       exclude_seen: bool = False, max_list_len: Optional[int] = None):
    """N3b stage 2 — co-occurrence candidates for many users at once: (ids int32[n, k] with -1 pads, scores float32[n, k],
    counts int32[n]).  max_list_len: the longest purchase list (sizes the workspace of the users whose terms do not fit
    LDS); read back from users_ptr when not given."""
    _need(users_ptr, t.int32, "users_ptr")
    _need(users_idx, t.int32, "users_idx")
    _need(nbr_id, t.int32, "nbr_id")
    _need(nbr_score, t.float32, "nbr_score")
    if nbr_id.dim() != 2 or nbr_id.shape != nbr_score.shape:
        raise ValueError("nbr_id and nbr_score must be [n_items, T] tables of one shape")
    if query_users is not None:
        _need(query_users, t.int64, "query_users")
        n_queries = query_users.numel()
    elif n_queries is None:
        n_queries = users_ptr.numel() - 1
    if n_recent is not None and int(n_recent) <= 0:
        raise ValueError("n_recent must be positive (None = the whole list)")
    if max_list_len is None:
        max_list_len = int((users_ptr[1:] - users_ptr[:-1]).max()) if users_ptr.numel() > 1 else 0
    T, k, dev = int(nbr_id.shape[1]), int(k), users_ptr.device
    L = _lib.lib()
    need = L.mi_match_cooc_workspace_bytes(n_queries, int(max_list_len), T)
    if need == 0 or k <= 0:
        raise ValueError(f"match_cooccurrence: k = {k} must be positive and T = {T} within 1..64")
    ws = _cooc_ws("match", need, dev)
    out = t.empty(n_queries, k, dtype=t.int32, device=dev)
    score = t.empty(n_queries, k, dtype=t.float32, device=dev)
    cnt = t.empty(n_queries, dtype=t.int32, device=dev)
    if n_queries and users_idx.numel() == 0:   # nobody holds anything: nothing to propose
        return out.fill_(-1), score.zero_(), cnt.zero_()
    check(L.mi_match_cooc_i32(n_queries, _ptr(query_users), users_ptr.data_ptr(), _ptr(users_idx), int(max_list_len), T,
                              _ptr(nbr_id), _ptr(nbr_score), k, int(n_recent or 0), int(bool(exclude_seen)),
                              _ptr(out), _ptr(score), _ptr(cnt), ws.data_ptr(), ws.numel(), _stream()), "mi_match_cooc_i32")
    return out, score, cnt


def check_random_walks(k, num_walks, walk_length, restart_prob, n_recent, boost) -> None:
    """The argument rules of the random-walk matcher (include/laplace_hip.h, N3c): ValueError naming the argument.  Needs no
    device; ops.match_random_walks, data.matching.RandomWalkMatcher and pinsage.evaluation.RandomWalkRecommender share it."""
    for name, v in (("k", k), ("num_walks", num_walks), ("walk_length", walk_length)):
        if isinstance(v, bool) or not isinstance(v, numbers.Integral) or v <= 0:
            raise ValueError(f"{name} must be a positive integer, got {v!r}")
    if isinstance(n_recent, bool) or not isinstance(n_recent, numbers.Integral) or not 1 <= n_recent <= _lib.MI_RECENT_MAX_SLOTS:
        raise ValueError(f"n_recent must be an integer in 1 .. {_lib.MI_RECENT_MAX_SLOTS}, got {n_recent!r}")
    try:
        ok = 0.0 <= float(restart_prob) < 1.0     # NaN fails both comparisons
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"restart_prob must be in [0, 1), got {restart_prob!r}")
    if boost not in _lib.MI_WALK_BOOSTS:
        raise ValueError(f"boost must be one of {sorted(_lib.MI_WALK_BOOSTS)}, got {boost!r}")
    if num_walks * walk_length > _lib.MI_WALK_MATCH_MAX_VISITS:
        raise ValueError(f"num_walks * walk_length = {num_walks * walk_length} is above the {_lib.MI_WALK_MATCH_MAX_VISITS} "
                         "visits one workgroup sorts")


def sort_csr_rows(ptr: Tensor, idx: Tensor) -> Tensor:
    """A copy of idx with every row of the int32 CSR (ptr, idx) sorted ascending: the table in which the random-walk matcher
    looks an item up with exclude_seen.  Built once per graph by its callers; row order itself stays the recency order."""
    _need(ptr, t.int32, "ptr")
    _need(idx, t.int32, "idx")
    rows = t.repeat_interleave(t.arange(ptr.numel() - 1, device=ptr.device), (ptr[1:] - ptr[:-1]).long())
    return (t.sort((rows << 31) | idx.long())[0] & 0x7FFFFFFF).to(t.int32)


def match_random_walks(iu_ptr: Tensor, iu_idx: Tensor, ui_ptr: Tensor, ui_idx: Tensor, k: int, *, num_walks: int, walk_length: int,
                       restart_prob: float, n_recent: int, boost: str, exclude_seen: bool, seed: int, step: int = 0,
                       n_queries: Optional[int] = None, query_users=None, ui_sorted: Optional[Tensor] = None):
    """N3c — random-walk (Pixie-style) candidates for many users at once: (ids int32[n, k] with -1 pads, scores float32[n, k]
    with 0 pads, counts int32[n] = distinct eligible items visited).  iu_*: item -> users, ui_*: user -> items in transaction
    order.  The rule is stated in include/laplace_hip.h; the draws are keyed on the user id, so a user's row is the same
    whoever else is queried.  query_users: int64 ids, any order, repeats allowed — a device tensor is taken as it is (an id
    outside the graph gets no proposal), ids on the host (list, array, CPU tensor) are checked and refused with ValueError.
    ui_sorted: ops.sort_csr_rows(ui_ptr, ui_idx), built here when exclude_seen needs it and the caller keeps none."""
    check_random_walks(k, num_walks, walk_length, restart_prob, n_recent, boost)
    if not 0 <= int(seed) < 2 ** 64 or not 0 <= int(step) < 2 ** 64:
        raise ValueError(f"seed and step must fit 64 unsigned bits, got {seed!r}, {step!r}")
    n_users = ui_ptr.numel() - 1
    if n_users < 0 or iu_ptr.numel() < 1:
        raise ValueError("ui_ptr and iu_ptr need n + 1 entries")
    if query_users is not None and not (isinstance(query_users, Tensor) and query_users.is_cuda):
        q = t.as_tensor(query_users).reshape(-1).to(t.int64)
        if q.numel() and (int(q.min()) < 0 or int(q.max()) >= n_users):
            raise ValueError(f"query_users must lie in [0, {n_users}), got ids from {int(q.min())} to {int(q.max())}")
        query_users = q.to(ui_ptr.device)
    if query_users is not None:
        n_queries = query_users.numel()
    elif n_queries is None:
        n_queries = n_users
    elif not 0 <= int(n_queries) <= n_users:
        raise ValueError(f"n_queries must lie in 0 .. {n_users}, got {n_queries!r}")
    for n, x in (("iu_ptr", iu_ptr), ("iu_idx", iu_idx), ("ui_ptr", ui_ptr), ("ui_idx", ui_idx)):
        _need(x, t.int32, n)
    if query_users is not None:
        _need(query_users, t.int64, "query_users")
    if iu_idx.numel() != ui_idx.numel():
        raise ValueError("iu_idx and ui_idx must list the same edges")
    if exclude_seen and ui_sorted is None:
        ui_sorted = sort_csr_rows(ui_ptr, ui_idx)
    if exclude_seen:
        _need(ui_sorted, t.int32, "ui_sorted")
        if ui_sorted.numel() != ui_idx.numel():
            raise ValueError("ui_sorted must be ui_idx with every row sorted")
    n_queries, k, dev = int(n_queries), int(k), ui_ptr.device
    ids = t.empty(n_queries, k, dtype=t.int32, device=dev)
    scores = t.empty(n_queries, k, dtype=t.float32, device=dev)
    counts = t.empty(n_queries, dtype=t.int32, device=dev)
    if n_queries and ui_idx.numel() == 0:   # nobody holds anything: nothing to propose
        return ids.fill_(-1), scores.zero_(), counts.zero_()
    check(_lib.lib().mi_match_random_walks_i32(n_queries, _ptr(query_users), n_users, iu_ptr.numel() - 1, iu_ptr.data_ptr(),
                                               _ptr(iu_idx), ui_ptr.data_ptr(), _ptr(ui_idx),
                                               _ptr(ui_sorted) if exclude_seen else None, k, int(num_walks), int(walk_length),
                                               float(restart_prob), int(n_recent), _lib.MI_WALK_BOOSTS[boost],
                                               int(bool(exclude_seen)), int(seed), int(step), _ptr(ids), _ptr(scores),
                                               _ptr(counts), _stream()), "mi_match_random_walks_i32")
    return ids, scores, counts


ALS_MAX_DIM = 128


def check_als(d, alpha, reg) -> None:
    """The argument rules of the implicit-ALS row solves (include/laplace_hip.h, iALS): ValueError naming the constraint.
    Needs no device; ops.als_solve_rows and als.ImplicitALS share it."""
    if isinstance(d, bool) or not isinstance(d, numbers.Integral):
        raise ValueError(f"dim must be an integer, got {d!r}")
    if d % 4 != 0:
        raise ValueError(f"dim must be a multiple of 4 (factor rows are read as float4), got {d}")
    if not 4 <= d <= ALS_MAX_DIM:
        raise ValueError(f"dim must lie in 4 .. {ALS_MAX_DIM} (one d x d system per workgroup, in LDS), got {d}")
    for name, v, strict in (("alpha", alpha, False), ("reg", reg, True)):
        try:
            v = float(v)
            ok = math.isfinite(v) and (v > 0.0 if strict else v >= 0.0)
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError(f"{name} must be a finite number {'> 0' if strict else '>= 0'}, got {v!r}")


def check_als_weights(nnz: int, n_rows: int, conf, reg_rows) -> None:
    """Shape and dtype of the per-entry confidences and per-row regularisers of the weighted row solves (include/laplace_hip.h,
    iALS weighted): conf float32 [nnz] by entry position, reg_rows float32 [n_rows] by row id; None passes.  ValueError
    naming which.  Needs no device and reads no value: the kernels treat a bad VALUE as a failed row."""
    for name, x, n, what in (("conf", conf, nnz, "nnz"), ("reg_rows", reg_rows, n_rows, "n_rows")):
        if x is None:
            continue
        if not isinstance(x, Tensor) or x.dtype != t.float32:
            raise ValueError(f"{name} must be a float32 tensor [{what}], got {getattr(x, 'dtype', type(x))}")
        if x.dim() != 1 or x.numel() != n:
            raise ValueError(f"{name} must have shape [{what}] = [{n}], got {tuple(x.shape)}")


def _als_weights(a: "DeviceCSR", conf, reg_rows, alpha: float, device) -> Tuple[Tensor, Optional[Tensor]]:
    """The device operands of a weighted call: conf filled with alpha where only reg_rows was given."""
    if conf is None:
        conf = t.full((a.nnz,), float(alpha), dtype=t.float32, device=device)
    _need(conf, t.float32, "conf")
    if reg_rows is not None:
        _need(reg_rows, t.float32, "reg_rows")
    return conf, reg_rows


def als_chunk(d: int) -> int:
    """L of the iALS rule for width d: entries per chunk of a row's rank-n update (mi_als_chunk)."""
    return int(_lib.lib().mi_als_chunk(int(d)))


def als_solve_rows(a: DeviceCSR, Y: Tensor, G: Tensor, *, alpha: float, reg: float, out: Optional[Tensor] = None,
                   row_list: Optional[Tensor] = None, conf: Optional[Tensor] = None,
                   reg_rows: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """iALS — for every row r of `a` (a CSR over the rows of Y [n_cols, d]) the solution of
    (G + alpha * sum_e y_e y_e^T + reg I) x = (1 + alpha) * sum_e y_e, f32 Cholesky, one workgroup per row; the rule is stated in
    include/laplace_hip.h.  G [d, d] is the caller's (the trainer passes gemm(Y, Y, trans_a=True, trans_b=False)).  Returns
    (X, n_failed): X [n_rows, d], or [len(row_list), d] compact by list position; n_failed an int32 device scalar counting the
    rows whose factorisation met a non-positive or non-finite pivot (those rows are zero).  Empty rows are zero and not counted.
    conf [nnz] (a_e by entry position of a.col) and / or reg_rows [n_rows] (by row id, also with a row_list) select the weighted
    entry, (G + sum_e a_e y_e y_e^T + reg_r I) x = sum_e (1 + a_e) y_e ("iALS weighted" in the header): conf=None is a_e = alpha,
    reg_rows=None is reg_r = reg; with conf given alpha is checked and not used.  With both None this is the unweighted
    entry, its call and its bits."""
    weighted = conf is not None or reg_rows is not None
    if weighted:
        check_als_weights(a.nnz, a.n_rows, conf, reg_rows)
    _need(a.rowptr, t.int32, "a.rowptr")
    _need(a.col, t.int32, "a.col")
    ldy = _rows_ok(Y, "Y")
    _need(G, t.float32, "G")
    if Y.shape[0] != a.n_cols:
        raise ValueError(f"Y must have one row per column of a: {a.n_cols}, got {Y.shape[0]}")
    d = int(Y.shape[1])
    check_als(d, alpha, reg)
    if tuple(G.shape) != (d, d):
        raise ValueError(f"G must be [{d}, {d}], got {tuple(G.shape)}")
    if a.rowptr.numel() != a.n_rows + 1:
        raise ValueError("a.rowptr needs n_rows + 1 entries")
    if row_list is not None:
        _need(row_list, t.int32, "row_list")
    n_work = int(row_list.numel()) if row_list is not None else a.n_rows
    if out is None:
        out = t.empty(n_work, d, dtype=t.float32, device=Y.device)
    ldx = _rows_ok(out, "out")
    if tuple(out.shape) != (n_work, d):
        raise ValueError(f"out must be [{n_work}, {d}], got {tuple(out.shape)}")
    n_failed = t.zeros(1, dtype=t.int32, device=Y.device)
    if n_work == 0 or a.nnz == 0:   # nothing to solve: every row is empty
        return out.zero_(), n_failed
    L = _lib.lib()
    if weighted:
        conf, reg_rows = _als_weights(a, conf, reg_rows, alpha, Y.device)
        ws = _ws_reused(L.mi_als_solve_rows_w_workspace_bytes(n_work, a.nnz, d), Y.device)
        check(L.mi_als_solve_rows_w_f32(a.n_rows, d, a.rowptr.data_ptr(), _ptr(a.col), a.nnz, a.n_cols, Y.data_ptr(), ldy,
                                        G.data_ptr(), conf.data_ptr(), _ptr(reg_rows), float(reg), out.data_ptr(), ldx,
                                        row_list.data_ptr() if row_list is not None else None,
                                        n_work if row_list is not None else 0, n_failed.data_ptr(), ws.data_ptr(), ws.numel(),
                                        _stream()), "mi_als_solve_rows_w_f32")
        return out, n_failed
    ws_bytes = L.mi_als_solve_rows_workspace_bytes(n_work, a.nnz, d)
    ws = _ws_reused(ws_bytes, Y.device)
    # a pointer that is never dereferenced where the tensor is empty (no entries, no listed rows) keeps the null check simple
    check(L.mi_als_solve_rows_f32(a.n_rows, d, a.rowptr.data_ptr(), _ptr(a.col), a.nnz, a.n_cols, Y.data_ptr(), ldy,
                                  G.data_ptr(), float(alpha), float(reg), out.data_ptr() if n_work else None, ldx,
                                  row_list.data_ptr() if row_list is not None else None, n_work if row_list is not None else 0,
                                  n_failed.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "mi_als_solve_rows_f32")
    return out, n_failed


ALS_BLOCK_MAX_DIM = 256
ALS_BLOCKS = (16, 32, 64)
ALS_BLOCK_MAX_SWEEPS = 64


def check_als_block(d, block, sweeps, alpha, reg) -> None:
    """The argument rules of the block row solver (include/laplace_hip.h, iALS block): ValueError naming the constraint.
    Needs no device; ops.als_block_rows and als.ImplicitALS share it."""
    if isinstance(d, bool) or not isinstance(d, numbers.Integral):
        raise ValueError(f"dim must be an integer, got {d!r}")
    if d % 4 != 0:
        raise ValueError(f"dim must be a multiple of 4 (factor rows are read as float4), got {d}")
    if not 4 <= d <= ALS_BLOCK_MAX_DIM:
        raise ValueError(f"dim must lie in 4 .. {ALS_BLOCK_MAX_DIM} for the block solver, got {d}")
    if isinstance(block, bool) or block not in ALS_BLOCKS:
        raise ValueError(f"block must be one of {ALS_BLOCKS}, got {block!r}")
    if isinstance(sweeps, bool) or not isinstance(sweeps, numbers.Integral) or not 1 <= sweeps <= ALS_BLOCK_MAX_SWEEPS:
        raise ValueError(f"sweeps must be an integer in 1 .. {ALS_BLOCK_MAX_SWEEPS}, got {sweeps!r}")
    check_als(4, alpha, reg)


def als_block_chunk(d: int, block: int) -> int:
    """The longest row that the block solver keeps on chip at width d (mi_als_block_chunk); 0 for a refused shape."""
    return int(_lib.lib().mi_als_block_chunk(int(d), int(block)))


def check_als_hub_threshold(hub_threshold, solver: str = "block") -> None:
    """hub_threshold of the block row solver (include/laplace_hip.h, iALS block hub): None, or an integer >= 1, and None for
    any solver but "block".  ValueError naming the argument; needs no device."""
    if hub_threshold is None:
        return
    if isinstance(hub_threshold, bool) or not isinstance(hub_threshold, numbers.Integral) or hub_threshold < 1:
        raise ValueError(f"hub_threshold must be None or an integer >= 1, got {hub_threshold!r}")
    if solver != "block":
        raise ValueError(f"hub_threshold is the block solver's: it must be None with solver={solver!r}, got {hub_threshold!r}")


def als_block_hub_chunk(d: int) -> int:
    """L_h of the hub rule for width d: entries per chunk of a hub row's Gram (mi_als_block_hub_chunk); 0 for a refused width."""
    return int(_lib.lib().mi_als_block_hub_chunk(int(d)))


def als_hub_counts(a: DeviceCSR, hub_threshold: int, d: int) -> Tuple[int, int]:
    """(rows of `a` with more than hub_threshold entries, sum over them of ceil(n / L_h)): what the hub entries size their
    workspace by.  One device reduction and one read-back per (CSR, threshold, chunk), kept on the CSR like its plans."""
    L = als_block_hub_chunk(d)
    key = (int(hub_threshold), L)
    if key not in a.hub_counts:
        n = (a.rowptr[1:] - a.rowptr[:-1]).long()
        hub = n > int(hub_threshold)
        chunks = t.where(hub, (n + (L - 1)) // L, t.zeros_like(n))
        a.hub_counts[key] = tuple(int(v) for v in t.stack([hub.sum(), chunks.sum()]).tolist())
    return a.hub_counts[key]


def als_block_rows(a: DeviceCSR, Y: Tensor, G: Tensor, *, alpha: float, reg: float, block: int = 16, sweeps: int = 1,
                   x: Optional[Tensor] = None, row_list: Optional[Tensor] = None, conf: Optional[Tensor] = None,
                   reg_rows: Optional[Tensor] = None, hub_threshold: Optional[int] = None) -> Tuple[Tensor, Tensor]:
    """iALS block — for every row r of `a` (a CSR over the rows of Y [n_cols, d]), `sweeps` passes over the blocks of `block`
    coordinates, each step the exact minimiser over its block of the row's quadratic
    1/2 x^T (G + alpha * sum_e y_e y_e^T + reg I) x - (1 + alpha) * sum_e y_e . x; one wavefront per row; the rule is stated
    in include/laplace_hip.h.  x [n_rows, d] (or [len(row_list), d], compact by list position) is the start and is UPDATED
    IN PLACE; x=None starts from zero into a fresh tensor.  Returns (X, n_failed) as als_solve_rows does.  conf / reg_rows: as
    in als_solve_rows, selecting the "iALS block weighted" entry; with both None the unweighted entry, its call and its bits.
    hub_threshold: None launches exactly that; an integer >= 1 selects the "iALS block hub" entries, which take every row with
    MORE entries from its d x d system, assembled once over one workgroup per chunk of the row (als_hub_counts sizes the
    workspace: one read-back per CSR and threshold); the other rows keep their bits."""
    check_als_hub_threshold(hub_threshold)
    weighted = conf is not None or reg_rows is not None
    if weighted:
        check_als_weights(a.nnz, a.n_rows, conf, reg_rows)
    _need(a.rowptr, t.int32, "a.rowptr")
    _need(a.col, t.int32, "a.col")
    ldy = _rows_ok(Y, "Y")
    _need(G, t.float32, "G")
    if Y.shape[0] != a.n_cols:
        raise ValueError(f"Y must have one row per column of a: {a.n_cols}, got {Y.shape[0]}")
    d = int(Y.shape[1])
    check_als_block(d, block, sweeps, alpha, reg)
    if tuple(G.shape) != (d, d):
        raise ValueError(f"G must be [{d}, {d}], got {tuple(G.shape)}")
    if a.rowptr.numel() != a.n_rows + 1:
        raise ValueError("a.rowptr needs n_rows + 1 entries")
    if row_list is not None:
        _need(row_list, t.int32, "row_list")
    n_work = int(row_list.numel()) if row_list is not None else a.n_rows
    from_zero = x is None
    if from_zero:
        x = t.empty(n_work, d, dtype=t.float32, device=Y.device)
    ldx = _rows_ok(x, "x")
    if tuple(x.shape) != (n_work, d):
        raise ValueError(f"x must be [{n_work}, {d}], got {tuple(x.shape)}")
    n_failed = t.zeros(1, dtype=t.int32, device=Y.device)
    if n_work == 0 or a.nnz == 0:   # nothing to solve: every row is empty
        return x.zero_(), n_failed
    L = _lib.lib()
    rl_ptr, n_list = (row_list.data_ptr(), n_work) if row_list is not None else (None, 0)
    if hub_threshold is not None:
        thr = min(int(hub_threshold), (1 << 31) - 1)
        hub_rows, hub_chunks = als_hub_counts(a, thr, d)   # over the whole CSR: upper bounds for a list of distinct rows
        if weighted:
            conf, reg_rows = _als_weights(a, conf, reg_rows, alpha, Y.device)
            ws = _ws_reused(L.mi_als_block_rows_hub_w_workspace_bytes(n_work, a.nnz, d, int(block), hub_rows, hub_chunks),
                            Y.device)
            check(L.mi_als_block_rows_hub_w_f32(a.n_rows, d, int(block), int(sweeps), a.rowptr.data_ptr(), _ptr(a.col), a.nnz,
                                                a.n_cols, Y.data_ptr(), ldy, G.data_ptr(), conf.data_ptr(), _ptr(reg_rows),
                                                float(reg), x.data_ptr(), ldx, int(from_zero), rl_ptr, n_list, thr, hub_rows,
                                                hub_chunks, n_failed.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
                  "mi_als_block_rows_hub_w_f32")
            return x, n_failed
        ws = _ws_reused(L.mi_als_block_rows_hub_workspace_bytes(n_work, a.nnz, d, int(block), hub_rows, hub_chunks), Y.device)
        check(L.mi_als_block_rows_hub_f32(a.n_rows, d, int(block), int(sweeps), a.rowptr.data_ptr(), _ptr(a.col), a.nnz,
                                          a.n_cols, Y.data_ptr(), ldy, G.data_ptr(), float(alpha), float(reg), x.data_ptr(), ldx,
                                          int(from_zero), rl_ptr, n_list, thr, hub_rows, hub_chunks, n_failed.data_ptr(),
                                          ws.data_ptr(), ws.numel(), _stream()), "mi_als_block_rows_hub_f32")
        return x, n_failed
    if weighted:
        conf, reg_rows = _als_weights(a, conf, reg_rows, alpha, Y.device)
        ws = _ws_reused(L.mi_als_block_rows_w_workspace_bytes(n_work, a.nnz, d, int(block)), Y.device)
        check(L.mi_als_block_rows_w_f32(a.n_rows, d, int(block), int(sweeps), a.rowptr.data_ptr(), _ptr(a.col), a.nnz,
                                        a.n_cols, Y.data_ptr(), ldy, G.data_ptr(), conf.data_ptr(), _ptr(reg_rows), float(reg),
                                        x.data_ptr(), ldx, int(from_zero), row_list.data_ptr() if row_list is not None else None,
                                        n_work if row_list is not None else 0, n_failed.data_ptr(), ws.data_ptr(), ws.numel(),
                                        _stream()), "mi_als_block_rows_w_f32")
        return x, n_failed
    ws_bytes = L.mi_als_block_rows_workspace_bytes(n_work, a.nnz, d, int(block))
    ws = _ws_reused(ws_bytes, Y.device)
    check(L.mi_als_block_rows_f32(a.n_rows, d, int(block), int(sweeps), a.rowptr.data_ptr(), _ptr(a.col), a.nnz, a.n_cols,
                                  Y.data_ptr(), ldy, G.data_ptr(), float(alpha), float(reg), x.data_ptr(), ldx, int(from_zero),
                                  row_list.data_ptr() if row_list is not None else None, n_work if row_list is not None else 0,
                                  n_failed.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "mi_als_block_rows_f32")
    return x, n_failed


_BN_WS = {}
BATCHNORM_MAX_CHANNELS = 512   # kBnMaxC of csrc/norm.hip: mi_batchnorm_*_f32 return MI_ERR_UNSUPPORTED beyond it


def _bn_ws(c: int, device) -> Tensor:
    key = (t.device(device).index, int(c))
    if key not in _BN_WS:
        _BN_WS[key] = _ws(_lib.lib().mi_batchnorm_workspace_bytes(int(c)), device)
    return _BN_WS[key]


def batchnorm_fwd(x: Tensor, gamma: Optional[Tensor], beta: Optional[Tensor], running_mean: Optional[Tensor],
                  running_var: Optional[Tensor], momentum: float, eps: float, training: bool):
    """K8 — BatchNorm1d over the rows of x [n, c].  Returns (y, save_mean, save_invstd); the running statistics are
    updated in place in training mode (torch semantics: unbiased variance, momentum)."""
    ldx = _rows_ok(x, "x")
    n, c = x.shape
    y = t.empty(n, c, dtype=t.float32, device=x.device)
    sm = t.empty(c, dtype=t.float32, device=x.device) if training else None
    si = t.empty(c, dtype=t.float32, device=x.device) if training else None
    ws = _bn_ws(c, x.device)
    check(_lib.lib().mi_batchnorm_fwd_f32(n, c, _ptr(x), ldx, _ptr(gamma), _ptr(beta), _ptr(running_mean), _ptr(running_var),
                                          float(momentum), float(eps), 1 if training else 0, _ptr(sm), _ptr(si), _ptr(y), c,
                                          ws.data_ptr(), ws.numel(), _stream()), "mi_batchnorm_fwd_f32")
    return y, sm, si


def batchnorm_bwd(x: Tensor, dy: Tensor, gamma: Optional[Tensor], save_mean: Tensor, save_invstd: Tensor,
                  need_dx: bool = True, need_dw: bool = True):
    """(dx, dgamma, dbeta) of batchnorm_fwd in training mode."""
    ldx, ldy = _rows_ok(x, "x"), _rows_ok(dy, "dy")
    n, c = x.shape
    dx = t.empty(n, c, dtype=t.float32, device=x.device) if need_dx else None
    dg = t.empty(c, dtype=t.float32, device=x.device) if need_dw else None
    db = t.empty(c, dtype=t.float32, device=x.device) if need_dw else None
    ws = _bn_ws(c, x.device)
    check(_lib.lib().mi_batchnorm_bwd_f32(n, c, _ptr(x), ldx, _ptr(dy), ldy, _ptr(gamma), _ptr(save_mean), _ptr(save_invstd),
                                          _ptr(dx), c, _ptr(dg), _ptr(db), ws.data_ptr(), ws.numel(), _stream()),
          "mi_batchnorm_bwd_f32")
    return dx, dg, db


def bce_logits(logits: Tensor, labels: Tensor, want_grad: bool = True):
    """b9 — BCEWithLogitsLoss(mean)(logits, labels) and d loss / d logits in one launch: (loss[1], dlogits or None)."""
    _need(logits, t.float32, "logits")
    _need(labels, t.float32, "labels")
    n = logits.numel()
    if labels.numel() != n or n == 0:
        raise ValueError("logits and labels must be non-empty and of equal length")
    loss = t.empty(1, dtype=t.float32, device=logits.device)
    dl = t.empty(n, dtype=t.float32, device=logits.device) if want_grad else None
    check(_lib.lib().mi_bce_logits_f32(n, _ptr(logits), _ptr(labels), _ptr(loss), _ptr(dl), _stream()), "mi_bce_logits_f32")
    return loss, dl


def gather_cat(zu: Tensor, zi: Tensor, row: Tensor, col: Tensor) -> Tensor:
    """b7 — cat(zu[row], zi[col], dim=-1) in one launch (model/encoder_decoder.py:57-63)."""
    _need(row, t.int64, "row")
    _need(col, t.int64, "col")
    ldu, ldi = _rows_ok(zu, "zu"), _rows_ok(zi, "zi")
    cu, ci, ne = zu.shape[1], zi.shape[1], row.numel()
    out = t.empty(ne, cu + ci, dtype=t.float32, device=zu.device)
    check(_lib.lib().mi_gather_cat_f32(ne, cu, ci, _ptr(row), _ptr(col), _ptr(zu), ldu, _ptr(zi), ldi, _ptr(out), cu + ci,
                                       _stream()), "mi_gather_cat_f32")
    return out


def gather_cat_bwd(d_out: Tensor, idx: Tensor, n_rows: int, c: int, off: int) -> Tensor:
    """dZ [n_rows, c]: rows of d_out[:, off:off+c] summed per idx value, in edge order (deterministic: no float
    atomics on either path)."""
    _need(idx, t.int64, "idx")
    ldo = _rows_ok(d_out, "d_out")
    ne = idx.numel()
    if ne > int(_lib.lib().mi_gather_cat_bwd_max_edges()):
        # beyond the all-pairs kernel's range: the same sum as a product with the [n_rows, ne] incidence matrix — a sorted
        # CSR (columns = edge positions, ascending) through the SpMM kernel, i.e. still summed in edge order
        if c % 4 or off % 4 or ldo % 4:
            raise ValueError("gather_cat_bwd beyond mi_gather_cat_bwd_max_edges needs widths / offsets that are multiples of 4")
        inc = coo_to_csr(idx.contiguous(), t.arange(ne, dtype=t.int64, device=idx.device), n_rows, ne, want_perm=False)
        inc.val = t.ones(ne, dtype=t.float32, device=idx.device)
        dz = t.empty(n_rows, c, dtype=t.float32, device=d_out.device)
        spmm(inc, d_out[:, off:off + c], Y=dz)
        return dz
    dz = t.zeros(n_rows, c, dtype=t.float32, device=d_out.device)
    check(_lib.lib().mi_gather_cat_bwd_f32(ne, c, off, _ptr(idx), _ptr(d_out), ldo, _ptr(dz), c, _stream()),
          "mi_gather_cat_bwd_f32")
    return dz


def sage_wgrad(problems) -> bool:
    """Weight gradients of up to four SAGEConv relations in one launch pair (mi_sage_wgrad_f32).  problems: dicts(dy [k, m],
    mask [k, m] or None, b1 [k, n1], b2 [k, n2] or None, gw1 [m, n1], gb [m] or None, gw2 [m, n2] or None), all contiguous
    float32.  False (nothing enqueued) when the shapes are outside the kernel's: the caller uses the grouped GEMM."""
    n = len(problems)
    if n == 0 or n > 4:
        return False
    arr = (_lib.WgradProblem * n)()
    for q, s in zip(arr, problems):
        dy, b1, b2 = s["dy"], s["b1"], s.get("b2")
        tensors = [dy, b1, s["gw1"]] + [x for x in (s.get("mask"), b2, s.get("gb"), s.get("gw2")) if x is not None]
        if any(x.dtype != t.float32 or not x.is_contiguous() for x in tensors) or (b2 is None) != (s.get("gw2") is None):
            return False
        if dy.dim() != 2 or b1.dim() != 2 or b1.shape[0] != dy.shape[0] or (b2 is not None and b2.shape[0] != dy.shape[0]):
            return False
        q.k, q.m, q.n1, q.n2 = int(dy.shape[0]), int(dy.shape[1]), int(b1.shape[1]), int(b2.shape[1]) if b2 is not None else 0
        q.dy, q.mask, q.b1, q.b2 = _ptr(dy), _ptr(s.get("mask")), _ptr(b1), _ptr(b2)
        q.gw1, q.gb, q.gw2 = _ptr(s["gw1"]), _ptr(s.get("gb")), _ptr(s.get("gw2"))
    L = _lib.lib()
    if not L.mi_sage_wgrad_supported(arr, n):
        return False
    ws = t.empty(max(int(L.mi_sage_wgrad_workspace_bytes(arr, n)), 256), dtype=t.uint8, device=problems[0]["dy"].device)
    rc = L.mi_sage_wgrad_f32(arr, n, _ptr(ws), ws.numel(), _stream())
    if rc == _lib.MI_ERR_UNSUPPORTED:
        return False
    check(rc, "mi_sage_wgrad_f32")
    return True


def linear1_bwd(dy: Tensor, weight: Tensor, x: Tensor, need_dx: bool = True):
    """Backward of a Linear layer with one output feature (weight [1, in]): (dx [n, in] or None, dW [1, in], db [1]).
    mi_linear1_bwd_f32: deterministic band sums instead of three [n, 1]-shaped products."""
    _need(dy, t.float32, "dy"); _need(weight, t.float32, "weight")
    ldx = _rows_ok(x, "x")
    n, k = int(x.shape[0]), int(x.shape[1])
    if dy.numel() != n or weight.numel() != k or not dy.is_contiguous() or not weight.is_contiguous():
        raise ValueError("linear1_bwd: dy [n] / [n, 1], weight [1, in], x [n, in] expected")
    dev = x.device
    dx = t.empty(n, k, dtype=t.float32, device=dev) if need_dx else None
    gw = t.empty(1, k, dtype=t.float32, device=dev)
    gb = t.empty(1, dtype=t.float32, device=dev)
    L = _lib.lib()
    ws = t.empty(int(L.mi_linear1_bwd_workspace_bytes(n, k)), dtype=t.uint8, device=dev)
    check(L.mi_linear1_bwd_f32(n, k, _ptr(dy), _ptr(weight), _ptr(x), ldx, _ptr(dx) if need_dx else None, k, _ptr(gw), _ptr(gb),
                               _ptr(ws), ws.numel(), _stream()), "mi_linear1_bwd_f32")
    return dx, gw, gb


def batch_nodes(users: Tensor, pos: Tensor, neg: Tensor, n_users: int, n_nodes: int, *, gmap: Optional[Tensor] = None,
                nodes: Optional[Tensor] = None, count: Optional[Tensor] = None, ws: Optional[Tensor] = None):
    """Unique node set of a BPR batch (neg [B] or [B, M]): (gmap int32[n_nodes], nodes int32[(2+M)B], count int32[2] on
    device: count[0] = unique nodes, count[1] = unique user nodes, whose slots come first)."""
    B, dev = users.numel(), users.device
    n_neg = 1 if neg.dim() == 1 else check_n_neg(int(neg.shape[1]))
    if neg.numel() != B * n_neg:
        raise ValueError("neg must be [B] or [B, M]")
    for n, x in (("users", users), ("pos", pos), ("neg", neg)):
        _need(x, t.int64, n)
    gmap = gmap if gmap is not None else t.empty(n_nodes, dtype=t.int32, device=dev)
    nodes = nodes if nodes is not None else t.empty((2 + n_neg) * B, dtype=t.int32, device=dev)
    if nodes.numel() < (2 + n_neg) * B:
        raise ValueError("nodes must hold (2 + M) * B slots")
    count = count if count is not None else t.empty(2, dtype=t.int32, device=dev)
    L = _lib.lib()
    ws = ws if ws is not None else _ws(L.mi_batch_nodes_workspace_bytes(n_nodes), dev)
    if neg.dim() == 1:
        check(L.mi_batch_nodes_i32(B, n_users, n_nodes, _ptr(users), _ptr(pos), _ptr(neg), _ptr(gmap), _ptr(nodes),
                                   _ptr(count), ws.data_ptr(), ws.numel(), _stream()), "mi_batch_nodes_i32")
    else:
        check(L.mi_batch_nodes_ex_i32(B, n_neg, n_users, n_nodes, _ptr(users), _ptr(pos), _ptr(neg), _ptr(gmap),
                                      _ptr(nodes), _ptr(count), ws.data_ptr(), ws.numel(), _stream()),
              "mi_batch_nodes_ex_i32")
    return gmap, nodes, count


def gather_rows(dst: Tensor, src: Tensor, rows: Tensor, n_dev: Optional[Tensor] = None, accumulate: bool = False,
                scale: float = 1.0, begin_dev: Optional[Tensor] = None, row_offset: int = 0) -> None:
    """dst[i] = scale * ((accumulate ? dst[i] : 0) + src[rows[i] - row_offset]) for i in [*begin_dev, *n_dev).
    A bf16 src (a stored layer of the bf16 forward) is widened on the way: dst[i] = (accumulate ? dst[i] : 0) + float(src[rows[i]]),
    mi_gather_rows_bf16_f32; scale, begin_dev and row_offset keep their defaults there."""
    _need(rows, t.int32, "rows")
    if isinstance(src, Tensor) and src.dtype is t.bfloat16:
        if scale != 1.0 or begin_dev is not None or row_offset != 0:
            raise ValueError("gather_rows from a bf16 table takes no scale, begin_dev or row_offset")
        lds_, ldd = _rows_ok_bf16(src, "src"), _rows_ok(dst, "dst")
        if dst.shape[0] < rows.numel() or dst.shape[1] != src.shape[1]:
            raise ValueError("dst must be [len(rows), d]")
        if n_dev is not None:
            _need(n_dev, t.int32, "n_dev")
        check(_lib.lib().mi_gather_rows_bf16_f32(rows.numel(), _ptr(n_dev), src.shape[1], _ptr(rows), src.data_ptr(), lds_,
                                                 dst.data_ptr(), ldd, 1 if accumulate else 0, _stream()),
              "mi_gather_rows_bf16_f32")
        return
    lds_, ldd = _rows_ok(src, "src"), _rows_ok(dst, "dst")
    if dst.shape[0] < rows.numel() or dst.shape[1] != src.shape[1]:
        raise ValueError("dst must be [len(rows), d]")
    check(_lib.lib().mi_gather_rows_f32(rows.numel(), _ptr(n_dev), _ptr(begin_dev), src.shape[1], _ptr(rows),
                                        int(row_offset), src.data_ptr(), lds_, dst.data_ptr(), ldd,
                                        1 if accumulate else 0, float(scale), _stream()), "mi_gather_rows_f32")


def scatter_rows(dst: Tensor, src: Tensor, rows: Tensor, n_dev: Optional[Tensor] = None,
                 begin_dev: Optional[Tensor] = None, row_offset: int = 0) -> None:
    """dst[rows[i] - row_offset] = src[i] for i in [*begin_dev, *n_dev) (rows distinct)."""
    _need(rows, t.int32, "rows")
    lds_, ldd = _rows_ok(src, "src"), _rows_ok(dst, "dst")
    if src.shape[0] < rows.numel() or dst.shape[1] != src.shape[1]:
        raise ValueError("src must be [len(rows), d]")
    check(_lib.lib().mi_scatter_rows_f32(rows.numel(), _ptr(n_dev), _ptr(begin_dev), src.shape[1], _ptr(rows),
                                         int(row_offset), src.data_ptr(), lds_, dst.data_ptr(), ldd, _stream()),
          "mi_scatter_rows_f32")
