"""PinSAGE model — reference: pinsage/layers.py:121-203 (WeightedSAGEConv, SAGENet, ItemToItemScorer) and
pinsage/model.py:16-34 (PinSAGEModel.get_repr, hinge loss), with the trainable item-id feature the
reference assigns (pinsage/model.py:52-53) as the projector input.

With ItemFeatures the projector is the reference's LinearProjector over every feature column (pinsage/layers.py:14-46, 90-118:
an embedding table per integer column, a Linear over the float columns, the id as one more column, summed) on
mi_pinsage_project_f32 / mi_pinsage_project_bwd_f32 (csrc/pinsage_proj.hip): ItemFeatures, ItemProjector.  ItemProjector's
project / project_backward / clear_rows are the one place that issues the projector's C calls (the base part, the text part, their
workspaces), for the autograd path and for the native iteration (pinsage/native.py) alike; its descriptors are cached and follow a
replaced parameter or buffer (native_binding.PointerSnapshot).

Heavy ops on the HIP kernels: the Q / W products on mi_gemm_f32 (relu fused), the weighted
neighbourhood sum on mi_spmm_csr_f32 over the block's destination-sorted CSR with values
w_e / max(sum_e w_e, 1), the id-embedding lookup on mi_gather_rows_f32.  The row L2-normalisation,
the per-pair dot products and the hinge are torch ops on [batch]-sized tensors.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence, Tuple

import torch as t
import torch.nn.functional as F
from torch import Tensor, nn

from .. import _lib, ops
from ..model.layers import Linear
from ..native_binding import PointerSnapshot


class _EmbedRowsFn(t.autograd.Function):
    """weight[ids] on mi_gather_rows_f32; the (sparse) gradient is accumulated with index_add_ into a dense buffer, or, for a lazy
    table (sparse=True), returned as a torch.sparse_coo_tensor over the rows of `ids`, which torch.optim.SparseAdam takes."""

    @staticmethod
    def forward(ctx, weight: Tensor, ids: Tensor, sparse: bool = False):
        out = t.empty(ids.numel(), weight.shape[1], device=weight.device)
        ops.gather_rows(out, weight, ids.to(t.int32).contiguous())
        ctx.save_for_backward(ids)
        ctx.shape, ctx.sparse = weight.shape, bool(sparse)
        return out

    @staticmethod
    def backward(ctx, g: Tensor):
        (ids,) = ctx.saved_tensors
        if ctx.sparse:      # repeated ids stay repeated entries: SparseAdam coalesces (sums) them
            return t.sparse_coo_tensor(ids.reshape(1, -1), g.contiguous(), tuple(ctx.shape)), None, None
        gw = t.zeros(ctx.shape, device=g.device)
        gw.index_add_(0, ids, g.contiguous())
        return gw, None, None


class TextColumn:
    """One text column of every item as a bag of words — the input of the reference's BagOfWords (pinsage/layers.py:49-87).
    `tokens` int64 [n_items, L], padded on the right as torchtext pads; `lengths` int64 [n_items]: the first lengths[i]
    entries of row i are item i's bag, whatever stands behind them (pad_id, if given, is only recorded) is never read.
    Validated once here, because the kernels index the tables with the tokens unchecked, and converted to the CSR that
    mi_pinsage_text_f32 reads: `ptr` int64 [n_items + 1], `tok` int32 [sum of lengths] (one unused entry when every bag is
    empty, so that the pointer is never null).  ValueError for a wrong dtype or rank, a length outside [0, L], a token outside
    [0, vocab_size) among the first lengths[i].  One host read."""

    def __init__(self, tokens: Tensor, lengths: Tensor, vocab_size: int, pad_id: Optional[int] = None):
        if not isinstance(tokens, Tensor) or tokens.dtype != t.int64 or tokens.dim() != 2:
            raise ValueError("TextColumn: tokens must be an int64 [n_items, L] tensor")
        if not isinstance(lengths, Tensor) or lengths.dtype != t.int64 or lengths.dim() != 1:
            raise ValueError("TextColumn: lengths must be an int64 [n_items] tensor")
        if lengths.shape[0] != tokens.shape[0]:
            raise ValueError(f"TextColumn: tokens has {tokens.shape[0]} items, lengths {lengths.shape[0]}")
        if tokens.device != lengths.device:
            raise ValueError("TextColumn: tokens and lengths live on different devices")
        if tokens.shape[0] < 1:
            raise ValueError("TextColumn: no items")
        self.vocab_size = int(vocab_size)
        if self.vocab_size < 1 or self.vocab_size > 2 ** 31 - 1:
            raise ValueError("TextColumn: vocab_size must lie in [1, 2^31)")
        self.pad_id = None if pad_id is None else int(pad_id)
        L = int(tokens.shape[1])
        live = t.arange(L, device=tokens.device)[None, :] < lengths[:, None]
        tok = tokens[live]                                           # row-major: item by item, ascending position
        stats = t.stack([lengths.min(), lengths.max(), tok.min() if tok.numel() else lengths.new_zeros(()),
                         tok.max() if tok.numel() else lengths.new_zeros(())]).cpu().tolist()      # the one host read
        if stats[0] < 0 or stats[1] > L:
            raise ValueError(f"TextColumn: a length outside [0, {L}]")
        if stats[2] < 0 or stats[3] >= self.vocab_size:
            raise ValueError(f"TextColumn: a token outside [0, {self.vocab_size}) within its bag")
        self.n_items, self.max_len, self.nnz = int(tokens.shape[0]), int(stats[1]), int(tok.numel())
        ptr = t.zeros(self.n_items + 1, dtype=t.int64, device=tokens.device)
        t.cumsum(lengths, 0, out=ptr[1:])
        self.ptr = ptr
        self.tok = tok.to(t.int32).contiguous() if tok.numel() else t.zeros(1, dtype=t.int32, device=tokens.device)

    @property
    def device(self):
        return self.ptr.device

    def to(self, device) -> "TextColumn":
        out = object.__new__(TextColumn)
        out.__dict__.update(self.__dict__)
        out.ptr, out.tok = self.ptr.to(device), self.tok.to(device)
        return out

    @classmethod
    def from_strings(cls, texts: Sequence[str], min_freq: int = 1) -> Tuple["TextColumn", List[str]]:
        """Lower-case, split on whitespace, build the vocabulary — what the reference's Field(lower=True) + build_vocab do
        (pinsage/layers.py:39-44): itos = ["<unk>", "<pad>"] + the words seen at least min_freq times, most frequent first
        (ties alphabetically); rarer words map to <unk>.  Returns (column on the CPU, itos)."""
        from collections import Counter
        docs = [str(s).lower().split() for s in texts]
        if not docs:
            raise ValueError("TextColumn.from_strings: no texts")
        freq = Counter(w for d in docs for w in d)
        itos = ["<unk>", "<pad>"] + [w for w, c in sorted(freq.items(), key=lambda kv: (-kv[1], kv[0])) if c >= int(min_freq)]
        stoi = {w: i for i, w in enumerate(itos)}
        L = max(1, max(len(d) for d in docs))
        tokens = t.full((len(docs), L), 1, dtype=t.int64)
        for i, d in enumerate(docs):
            if d:
                tokens[i, : len(d)] = t.tensor([stoi.get(w, 0) for w in d], dtype=t.int64)
        return cls(tokens, t.tensor([len(d) for d in docs], dtype=t.int64), len(itos), pad_id=1), itos


def _pool_text(column: "TextColumn", table: Tensor) -> Tensor:
    """The mean of table's rows over every item's bag, [n_items, table.shape[1]]: mi_pinsage_text_f32 over the catalogue."""
    if not table.is_cuda or table.dtype != t.float32 or not table.is_contiguous() or column.device != table.device:
        raise _lib.MiError("text pooling: the table must be a contiguous float32 CUDA tensor on the column's device "
                           "(there is no CPU fallback)")
    d = _lib.TextColumns()
    d.width, d.n_text, d.n_items = int(table.shape[1]), 1, column.n_items
    d.ptr[0], d.tok[0], d.tables[0], d.vocab[0] = column.ptr.data_ptr(), column.tok.data_ptr(), table.data_ptr(), column.vocab_size
    out = t.empty(column.n_items, int(table.shape[1]), dtype=t.float32, device=table.device)
    _lib.check(_lib.lib().mi_pinsage_text_f32(ctypes.byref(d), column.n_items, None, out.data_ptr(), int(out.stride(0)), 0,
                                              _lib.current_stream()), "mi_pinsage_text_f32")
    return out


class ItemFeatures:
    """The feature columns of every item — what the reference's LinearProjector projects beside the id (pinsage/layers.py:14-46,
    90-118): `categorical` int64 [n_items, C] (0 <= C <= 16) codes, `dense` float32 [n_items, F], `text` up to 4 TextColumns
    (bags of words, keyword-only); at least one of them.
    cardinalities[c] defaults to categorical[:, c].max() + 1 (one host read).  The kernels index the tables with these codes
    unchecked, so they are checked once here: ValueError for a wrong dtype or rank, disagreeing item counts, a negative code
    or a code >= its cardinality."""

    def __init__(self, categorical: Optional[Tensor] = None, dense: Optional[Tensor] = None,
                 cardinalities: Optional[Sequence[int]] = None, *, text: Optional[Sequence[TextColumn]] = None):
        text = tuple(text) if text is not None else ()
        if any(not isinstance(c, TextColumn) for c in text):
            raise ValueError("ItemFeatures: text must be a sequence of TextColumn")
        if len(text) > _lib.MI_PROJECTOR_MAX_TEXT:
            raise ValueError(f"ItemFeatures: at most {_lib.MI_PROJECTOR_MAX_TEXT} text columns")
        self.text: Tuple[TextColumn, ...] = text
        if text:
            others = [x for x in (categorical, dense) if isinstance(x, Tensor)]
            if any(c.n_items != text[0].n_items for c in text) or any(x.dim() == 2 and x.shape[0] != text[0].n_items for x in others):
                raise ValueError("ItemFeatures: the text columns and the other features disagree on the number of items")
            if any(c.device != text[0].device for c in text) or any(x.device != text[0].device for x in others):
                raise ValueError("ItemFeatures: the text columns and the other features live on different devices")
        if categorical is None and dense is None and text:
            self.n_items = text[0].n_items
            self.categorical = self.dense = None
            if cardinalities is not None and len(cardinalities):
                raise ValueError("ItemFeatures: cardinalities without categorical columns")
            self.cardinalities: Tuple[int, ...] = ()
            return
        if categorical is None and dense is None:
            raise ValueError("ItemFeatures: give categorical, dense or both")
        if categorical is not None and (not isinstance(categorical, Tensor) or categorical.dtype != t.int64 or categorical.dim() != 2):
            raise ValueError("ItemFeatures: categorical must be an int64 [n_items, C] tensor")
        if dense is not None and (not isinstance(dense, Tensor) or dense.dtype != t.float32 or dense.dim() != 2):
            raise ValueError("ItemFeatures: dense must be a float32 [n_items, F] tensor")
        if categorical is not None and dense is not None and categorical.shape[0] != dense.shape[0]:
            raise ValueError(f"ItemFeatures: categorical has {categorical.shape[0]} items, dense {dense.shape[0]}")
        if categorical is not None and dense is not None and categorical.device != dense.device:
            raise ValueError("ItemFeatures: categorical and dense live on different devices")
        n_cols = 0 if categorical is None else int(categorical.shape[1])
        if n_cols > _lib.MI_PROJECTOR_MAX_COLS:
            raise ValueError(f"ItemFeatures: at most {_lib.MI_PROJECTOR_MAX_COLS} categorical columns")
        self.n_items = int((categorical if categorical is not None else dense).shape[0])
        if self.n_items < 1:
            raise ValueError("ItemFeatures: no items")
        self.categorical = categorical.contiguous() if n_cols else None
        self.dense = dense.contiguous() if dense is not None and dense.shape[1] > 0 else None
        if self.categorical is None and self.dense is None and not text:
            raise ValueError("ItemFeatures: no feature column (C = 0 and F = 0)")
        cards: List[int] = []
        if n_cols:
            lo, hi = self.categorical.min(0).values.cpu().tolist(), self.categorical.max(0).values.cpu().tolist()   # the one host read
            if min(lo) < 0:
                raise ValueError(f"ItemFeatures: negative code in column {lo.index(min(lo))}")
            cards = [int(h) + 1 for h in hi] if cardinalities is None else [int(c) for c in cardinalities]
            if len(cards) != n_cols:
                raise ValueError(f"ItemFeatures: {len(cards)} cardinalities for {n_cols} columns")
            for c, (h, card) in enumerate(zip(hi, cards)):
                if h >= card:
                    raise ValueError(f"ItemFeatures: code {h} in column {c} >= its cardinality {card}")
        elif cardinalities is not None and len(cardinalities):
            raise ValueError("ItemFeatures: cardinalities without categorical columns")
        self.cardinalities: Tuple[int, ...] = tuple(cards)

    @property
    def n_cols(self) -> int:
        return len(self.cardinalities)

    @property
    def n_dense(self) -> int:
        return 0 if self.dense is None else int(self.dense.shape[1])

    @property
    def n_text(self) -> int:
        return len(self.text)

    def with_pooled_text(self, column: TextColumn, vectors: Tensor) -> "ItemFeatures":
        """The reference's BagOfWordsPretrained (pinsage/layers.py:49-87): the mean of FROZEN word vectors, then a Linear.  The
        pooled vector of an item never changes, so it is computed once here — mi_pinsage_text_f32 over the catalogue at
        width = P — and appended to `dense`: a new ItemFeatures whose dense is [dense | pooled], everything else shared.
        `vectors` float32 [column.vocab_size, P] with P % 4 == 0 and 4 <= P <= 512 on the column's (CUDA) device; ValueError
        otherwise.  One Linear over [dense | pooled] equals the reference's sum of one Linear per input; only the
        xavier-uniform fan-in of its initial weights differs (F + P inputs instead of F and P apart)."""
        if not isinstance(column, TextColumn) or column.n_items != self.n_items:
            raise ValueError("ItemFeatures.with_pooled_text: a TextColumn over the same items expected")
        if not isinstance(vectors, Tensor) or vectors.dtype != t.float32 or vectors.dim() != 2 or vectors.shape[0] != column.vocab_size:
            raise ValueError("ItemFeatures.with_pooled_text: vectors must be float32 [vocab_size, P]")
        P = int(vectors.shape[1])
        if P % 4 or not (4 <= P <= 512):
            raise ValueError("ItemFeatures.with_pooled_text: P % 4 == 0 and 4 <= P <= 512 expected")
        pooled = _pool_text(column, vectors.contiguous())
        if self.dense is not None and self.dense.device != pooled.device:
            raise ValueError("ItemFeatures.with_pooled_text: dense and the pooled vectors live on different devices")
        dense = pooled if self.dense is None else t.cat([self.dense, pooled], 1)
        return ItemFeatures(self.categorical, dense, self.cardinalities if self.cardinalities else None, text=self.text)


class _ProjectFn(t.autograd.Function):
    """ItemProjector.forward on mi_pinsage_project_f32; the backward on mi_pinsage_project_bwd_f32 into fresh zero buffers of
    the parameters' shapes (dense table gradients, as _EmbedRowsFn's).  The gradient of a lazy table (PinSAGEModel(sparse_tables=
    True): the id table, the text tables) is handed on as a torch.sparse_coo_tensor over the rows the call REFERENCES — their
    summed rows out of the dense buffer, a row whose sum is exactly zero included — so that torch.optim.SparseAdam moves the
    rows the native step moves.  torch ops: this is the fallback path."""

    @staticmethod
    def forward(ctx, projector: "ItemProjector", ids: Optional[Tensor], *params: Tensor):
        ctx.projector, ctx.ids = projector, ids
        ctx.shapes = [p.shape for p in params]
        return projector.project(ids)

    @staticmethod
    def backward(ctx, g: Tensor):
        projector = ctx.projector
        grads = [t.zeros(s, dtype=t.float32, device=g.device) for s in ctx.shapes]
        projector.project_backward(ctx.ids, g.contiguous(), grads)
        if projector.sparse_tables:
            for k, rows in enumerate(projector.referenced_rows(ctx.ids)):
                if rows is not None:
                    grads[k] = t.sparse_coo_tensor(rows.reshape(1, -1), grads[k][rows], tuple(ctx.shapes[k]))
        return (None, None, *grads)


class _Bound:
    """What ItemProjector.bind() keeps: the two descriptors, the snapshot of the tensors they point into, the gradient descriptors
    of the last gradient buffers seen, and the workspaces with the row capacities they were sized for."""

    def __init__(self, projector: "ItemProjector"):
        self.base = projector.descriptor()
        self.text = projector.text_descriptor() if projector.n_text else None
        self.grads_of = self.grads_key = self.g_base = self.g_text = None
        self.ws, self.rows, self.text_ws = None, -1, {}      # text_ws: with_ids -> (row capacity, workspace, reference bound)
        self.snap = PointerSnapshot([projector.parameter_list, projector.feature_buffers])


class ItemProjector(nn.Module):
    """projector(ids) = id row (if the model has an id table) + one table row per categorical column, in column order,
    + dense[ids] @ W^T + b: one f32 addition chain in that order (mi_pinsage_project_f32).  Tables are [cardinality + 1,
    hidden] (the reference's max + 2 rows; the last row is never looked up), xavier-uniform; Linear(F, hidden) with
    xavier-uniform weight and zero bias.  The id table stays PinSAGEModel.proj (the same state_dict key as without features).
    Text columns come last in the chain: + the mean of text_tables[c]'s rows over the item's bag, in column order
    (mi_pinsage_text_f32; [vocab_size, hidden] xavier-uniform tables, drawn after every other parameter)."""

    def __init__(self, features: ItemFeatures, hidden_dims: int, id_embedding: Optional[nn.Embedding]):
        super().__init__()
        self.hidden, self.n_items = int(hidden_dims), features.n_items
        self.cardinalities = features.cardinalities
        self.tables = nn.ParameterList([nn.Parameter(t.empty(card + 1, hidden_dims)) for card in features.cardinalities])
        for tab in self.tables:
            nn.init.xavier_uniform_(tab)
        if features.n_dense:
            self.weight = nn.Parameter(t.empty(hidden_dims, features.n_dense))
            self.bias = nn.Parameter(t.zeros(hidden_dims))
            nn.init.xavier_uniform_(self.weight)
        else:
            self.weight = self.bias = None
        # buffers follow .to(device); not part of the state_dict (data, not weights)
        self.register_buffer("x", features.categorical, persistent=False)
        self.register_buffer("dense", features.dense, persistent=False)
        self._id = [id_embedding] if id_embedding is not None else []    # a list: PinSAGEModel.proj stays its only registration
        self.sparse_tables = False                 # PinSAGEModel(sparse_tables=True) sets it: the id and text tables are lazy
        self._bound: Optional["_Bound"] = None     # descriptors, workspaces and the pointers they were built from (bind)
        self.n_text = len(features.text)
        if self.n_text:
            self.text_tables = nn.ParameterList([nn.Parameter(t.empty(c.vocab_size, hidden_dims)) for c in features.text])
            for tab in self.text_tables:
                nn.init.xavier_uniform_(tab)
            for c, col in enumerate(features.text):
                self.register_buffer(f"text_ptr_{c}", col.ptr, persistent=False)
                self.register_buffer(f"text_tok_{c}", col.tok, persistent=False)
        self._text_buffers = tuple(f"text_{k}_{c}" for c in range(self.n_text) for k in ("ptr", "tok"))
        self.text_vocab = tuple(c.vocab_size for c in features.text)
        self.text_max_len = tuple(c.max_len for c in features.text)
        self.text_nnz = tuple(c.nnz for c in features.text)

    @property
    def id_weight(self) -> Optional[Tensor]:
        return self._id[0].weight if self._id else None

    def parameter_list(self) -> List[Tensor]:
        """[id table?] + tables + [W, b]? + text tables: the order of forward's chain, of _ProjectFn's gradients and of
        descriptor() / text_descriptor()."""
        out = [self.id_weight] if self._id else []
        out += list(self.tables)
        if self.weight is not None:
            out += [self.weight, self.bias]
        if self.n_text:
            out += list(self.text_tables)
        return out

    def lazy_flags(self) -> List[bool]:
        """Per parameter_list() entry: whether it is a lazy table (the id table and the text tables of a sparse_tables model;
        categorical tables are cardinality-sized — most rows are touched by every batch — and stay dense)."""
        n_mid = len(self.tables) + (2 if self.weight is not None else 0)
        return [self.sparse_tables] * len(self._id) + [False] * n_mid + [self.sparse_tables] * self.n_text

    def referenced_rows(self, ids: Optional[Tensor]) -> List[Optional[Tensor]]:
        """Per parameter_list() entry: the distinct rows (sorted int64) of a lazy table that project(ids) looks up — the items for
        the id table, the tokens of those items' bags for a text table — or None for a dense parameter.  torch ops."""
        dev = self.parameter_list()[0].device
        items = t.arange(self.n_items, device=dev) if ids is None else ids
        out: List[Optional[Tensor]] = []
        for k, lazy in enumerate(self.lazy_flags()):
            if not lazy:
                out.append(None)
            elif k < len(self._id):
                out.append(t.unique(items))
            else:
                c = k - (len(self.lazy_flags()) - self.n_text)
                ptr, tok = getattr(self, f"text_ptr_{c}"), getattr(self, f"text_tok_{c}")
                it = out[0] if (self._id and out[0] is not None) else t.unique(items)
                ln = ptr[it + 1] - ptr[it]
                rep = t.repeat_interleave(t.arange(it.numel(), device=dev), ln)
                pos = ptr[it][rep] + (t.arange(rep.numel(), device=dev) - (t.cumsum(ln, 0) - ln)[rep])
                out.append(t.unique(tok[pos].long()))
        return out

    @property
    def has_base(self) -> bool:
        """Anything for mi_pinsage_project_f32 (a text-only projector never calls it)."""
        return bool(self._id) or len(self.tables) > 0 or self.weight is not None

    def text_descriptor(self) -> "_lib.TextColumns":
        d = _lib.TextColumns()
        d.width, d.n_text, d.n_items = self.hidden, self.n_text, self.n_items
        for c, tab in enumerate(self.text_tables):
            ptr, tok = getattr(self, f"text_ptr_{c}"), getattr(self, f"text_tok_{c}")
            if tab.dtype != t.float32 or not tab.is_cuda or not tab.is_contiguous() or ptr.device != tab.device or tok.device != tab.device:
                raise _lib.MiError("ItemProjector: text tables must be contiguous float32 CUDA tensors on the text columns' device "
                                   "(there is no CPU fallback)")
            d.ptr[c], d.tok[c], d.tables[c], d.vocab[c] = ptr.data_ptr(), tok.data_ptr(), tab.data_ptr(), int(tab.shape[0])
        return d

    def text_grads(self, grads: Sequence[Tensor]) -> "_lib.TextGradTables":
        """The g_tables argument of the text entries from `grads` (parameter_list() order: the text tables are its tail)."""
        arr = _lib.TextGradTables()
        for c, g in enumerate(list(grads)[len(grads) - self.n_text:]):
            arr[c] = g.data_ptr()
        return arr

    def text_ref_bound(self, n: int, with_ids: bool) -> int:
        """An upper bound of the references of a call over n rows: n times the longest bags; without ids (rows 0 .. n - 1,
        each once) also the columns' token counts."""
        bound = n * sum(self.text_max_len)
        return bound if with_ids else min(bound, sum(self.text_nnz))

    def descriptor(self) -> "_lib.ItemProjector":
        d = _lib.ItemProjector()
        params = self.parameter_list()
        if any(p.dtype != t.float32 or not p.is_cuda or not p.is_contiguous() for p in params):
            raise _lib.MiError("ItemProjector: parameters must be contiguous float32 CUDA tensors (there is no CPU fallback)")
        if any(b is not None and (not b.is_cuda or b.device != params[0].device) for b in (self.x, self.dense)):
            raise _lib.MiError("ItemProjector: the feature tensors must live on the parameters' device")
        d.hidden, d.n_cols, d.n_items = self.hidden, len(self.tables), self.n_items
        d.x = self.x.data_ptr() if self.x is not None else None
        for c, tab in enumerate(self.tables):
            d.tables[c], d.table_rows[c] = tab.data_ptr(), int(tab.shape[0])
        d.id_table = self.id_weight.data_ptr() if self._id else None
        if self.weight is not None:
            d.n_dense, d.dense, d.ld_dense = int(self.dense.shape[1]), self.dense.data_ptr(), int(self.dense.stride(0))
            d.w, d.b = self.weight.data_ptr(), self.bias.data_ptr()
        return d

    def grads_descriptor(self, grads: Sequence[Tensor]) -> "_lib.ItemProjectorGrads":
        """grads: one buffer per parameter_list() entry, each with its parameter's shape."""
        gd = _lib.ItemProjectorGrads()
        grads = list(grads)
        if len(grads) != len(self.parameter_list()) or any(
                g.shape != p.shape or g.dtype != t.float32 or not g.is_contiguous() for g, p in zip(grads, self.parameter_list())):
            raise ValueError("ItemProjector: gradient buffers must be contiguous float32 of their parameters' shapes")
        if self._id:
            gd.g_id_table = grads.pop(0).data_ptr()
        for c in range(len(self.tables)):
            gd.g_tables[c] = grads.pop(0).data_ptr()
        if self.weight is not None:
            gd.g_w, gd.g_b = grads[0].data_ptr(), grads[1].data_ptr()
        return gd

    # ---- the C calls.  This is the one place that knows the base / text branching, the two workspaces and the reference bound:
    # the autograd path (forward / _ProjectFn.backward) and pinsage.native.NativePinSAGEStep both come through here. ----------------
    def feature_buffers(self) -> tuple:
        """The data the descriptors point to beside the parameters, each replaceable on its own."""
        return (self.x, self.dense) + tuple(getattr(self, name) for name in self._text_buffers)

    def __getstate__(self):    # a copy or a pickle starts without the cache: raw pointers into THIS module's tensors
        return {**self.__dict__, "_bound": None}

    def bind(self) -> "_Bound":
        """The descriptors, built once and again when a parameter or a buffer was replaced (.to(device), a new code matrix);
        the gradient descriptors and the workspaces are dropped with them.  A caller that knows by itself when that happens
        (the native step: its own snapshot covers the same tensors) binds once and hands the result to the three calls below
        as `bound`, which then check nothing."""
        b = self._bound
        if b is None or not b.snap.current():
            b = self._bound = _Bound(self)
        return b

    def _grads(self, b: "_Bound", grads: Sequence[Tensor]):
        """(mi_item_projector_grads, the text entries' g_tables) over `grads`, kept for as long as the same buffers come.  The
        same TUPLE again (the native step's, made when its descriptor is built) is taken by identity; any other sequence by
        its addresses (the autograd path brings fresh buffers with every backward)."""
        if type(grads) is not tuple or grads is not b.grads_of:
            key = tuple(g.data_ptr() for g in grads)
            if key != b.grads_key:
                b.grads_key, b.g_base, b.g_text = key, self.grads_descriptor(grads), self.text_grads(grads) if self.n_text else None
            b.grads_of = grads
        return b.g_base, b.g_text

    def _workspace(self, b: "_Bound", n: int) -> Tensor:
        """Of mi_pinsage_project_f32 and its backward, sized for a row capacity: the C size queries run when n exceeds it."""
        if n > b.rows:
            L, pd, rows = _lib.lib(), ctypes.byref(b.base), max(1024, int(n * 1.25))
            need = max(int(L.mi_pinsage_project_workspace_bytes(pd, rows)), int(L.mi_pinsage_project_bwd_workspace_bytes(pd, rows)))
            b.ws, b.rows = t.empty(need, dtype=t.uint8, device=self.parameter_list()[0].device), rows
        return b.ws

    def _text_workspace(self, b: "_Bound", n: int, with_ids: bool) -> Tuple[Tensor, int]:
        """(workspace, reference bound) of mi_pinsage_text_bwd_f32: the bound is text_ref_bound of the row capacity, one capacity
        for calls with ids and one for calls without."""
        have = b.text_ws.get(with_ids)
        if have is None or n > have[0]:
            rows = max(1024, int(n * 1.25))
            ref_max = self.text_ref_bound(rows, with_ids)
            need = int(_lib.lib().mi_pinsage_text_bwd_workspace_bytes(ctypes.byref(b.text), rows, ref_max))
            have = b.text_ws[with_ids] = (rows, t.empty(need, dtype=t.uint8, device=self.parameter_list()[0].device), ref_max)
        return have[1], have[2]

    def _rows_of(self, ids: Optional[Tensor], n: Optional[int] = None):
        """(the ids, contiguous; their count; their address): rows `ids`, or None for items 0 .. n - 1 (n = n_items by default)."""
        if ids is None:
            return None, (self.n_items if n is None else int(n)), None
        if ids.dtype != t.int64 or ids.dim() != 1 or not ids.is_cuda:
            raise _lib.MiError("ItemProjector: ids must be a 1-d int64 CUDA tensor")
        ids = ids.contiguous()
        return ids, int(ids.numel()), ids.data_ptr()

    def project(self, ids: Optional[Tensor], out: Optional[Tensor] = None, n: Optional[int] = None,
                bound: Optional["_Bound"] = None) -> Tensor:
        """The forward with no autograd: rows of `ids` (None: items 0 .. n - 1, n = n_items by default) into the first n rows of
        out [>= n, hidden]."""
        ids, n, idp = self._rows_of(ids, n)
        b, L, stream = bound or self.bind(), _lib.lib(), _lib.current_stream()
        if out is None:
            out = t.empty(n, self.hidden, dtype=t.float32, device=self.parameter_list()[0].device)
        ldo = int(out.stride(0)) if n else self.hidden
        if self.has_base:
            ws = self._workspace(b, n)
            _lib.check(L.mi_pinsage_project_f32(ctypes.byref(b.base), n, idp, out.data_ptr(), ldo, ws.data_ptr(), ws.numel(), stream),
                       "mi_pinsage_project_f32")
        if self.n_text:
            _lib.check(L.mi_pinsage_text_f32(ctypes.byref(b.text), n, idp, out.data_ptr(), ldo, 1 if self.has_base else 0, stream),
                       "mi_pinsage_text_f32")
        return out

    def project_backward(self, ids: Optional[Tensor], g: Tensor, grads: Sequence[Tensor], bound: Optional["_Bound"] = None) -> None:
        """g = dL/d project(ids), the first n rows of [>= n, hidden], into `grads` (parameter_list() order): looked-up table rows
        are written, others left."""
        ids, n, idp = self._rows_of(ids)
        b, L, stream = bound or self.bind(), _lib.lib(), _lib.current_stream()
        gd, tg = self._grads(b, grads)
        ldg = int(g.stride(0)) if n else self.hidden
        if self.has_base:
            ws = self._workspace(b, n)
            _lib.check(L.mi_pinsage_project_bwd_f32(ctypes.byref(b.base), ctypes.byref(gd), n, idp, g.data_ptr(), ldg, ws.data_ptr(),
                                                    ws.numel(), stream), "mi_pinsage_project_bwd_f32")
        if self.n_text:
            ws, ref_max = self._text_workspace(b, n, ids is not None)
            _lib.check(L.mi_pinsage_text_bwd_f32(ctypes.byref(b.text), tg, n, idp, g.data_ptr(), ldg, ref_max, ws.data_ptr(), ws.numel(),
                                                 stream), "mi_pinsage_text_bwd_f32")

    def project_backward_lazy(self, ids: Optional[Tensor], g: Tensor, grads: Sequence[Tensor], moments: Sequence,
                              lazy: Sequence["_lib.LazyAdam"], bound: Optional["_Bound"] = None) -> None:
        """project_backward, then torch.optim.SparseAdam's update of every referenced row of the lazy tables in the same calls
        (mi_pinsage_project_bwd_lazy_f32, mi_pinsage_text_bwd_lazy_f32).  moments: per parameter_list() entry (exp_avg, exp_avg_sq)
        for a lazy table, None otherwise; lazy = (the id table's hyper-parameters and step, the text tables').  A lazy table's
        buffer in `grads` reads zero again afterwards; the others hold their gradients as after project_backward."""
        ids, n, idp = self._rows_of(ids)
        b, L, stream = bound or self.bind(), _lib.lib(), _lib.current_stream()
        gd, tg = self._grads(b, grads)
        ldg = int(g.stride(0)) if n else self.hidden
        moments = list(moments)
        if self.has_base:
            mo = _lib.ItemProjectorMoments()
            if self._id and moments[0] is not None:
                mo.m_id_table, mo.v_id_table = moments[0][0].data_ptr(), moments[0][1].data_ptr()
            for c, pair in enumerate(moments[len(self._id): len(self._id) + len(self.tables)]):
                if pair is not None:       # a categorical table is dense in every model of this package; the entry takes either
                    mo.m_tables[c], mo.v_tables[c] = pair[0].data_ptr(), pair[1].data_ptr()
            ws = self._workspace(b, n)
            _lib.check(L.mi_pinsage_project_bwd_lazy_f32(ctypes.byref(b.base), ctypes.byref(gd), ctypes.byref(mo), ctypes.byref(lazy[0]),
                                                         n, idp, g.data_ptr(), ldg, ws.data_ptr(), ws.numel(), stream),
                       "mi_pinsage_project_bwd_lazy_f32")
        if self.n_text:
            mt, vt = _lib.TextGradTables(), _lib.TextGradTables()
            for c, pair in enumerate(moments[len(moments) - self.n_text:]):
                if pair is not None:
                    mt[c], vt[c] = pair[0].data_ptr(), pair[1].data_ptr()
            ws, ref_max = self._text_workspace(b, n, ids is not None)
            _lib.check(L.mi_pinsage_text_bwd_lazy_f32(ctypes.byref(b.text), tg, mt, vt, ctypes.byref(lazy[1]), n, idp, g.data_ptr(), ldg,
                                                      ref_max, ws.data_ptr(), ws.numel(), stream), "mi_pinsage_text_bwd_lazy_f32")

    def clear_rows(self, ids: Optional[Tensor], grads: Sequence[Tensor], bound: Optional["_Bound"] = None, text: bool = True) -> None:
        """The table rows project_backward(ids, ...) wrote, back to zero (mi_pinsage_project_clear_f32); text=False leaves the text
        tables' buffers out (the lazy backward has zeroed them itself)."""
        ids, n, idp = self._rows_of(ids)
        b, L, stream = bound or self.bind(), _lib.lib(), _lib.current_stream()
        gd, tg = self._grads(b, grads)
        if self.has_base:
            _lib.check(L.mi_pinsage_project_clear_f32(ctypes.byref(b.base), ctypes.byref(gd), n, idp, stream),
                       "mi_pinsage_project_clear_f32")
        if self.n_text and text:
            _lib.check(L.mi_pinsage_text_clear_f32(ctypes.byref(b.text), tg, n, idp, stream), "mi_pinsage_text_clear_f32")

    def forward(self, ids: Optional[Tensor] = None) -> Tensor:
        return _ProjectFn.apply(self, ids, *self.parameter_list())


class _WeightedSumFn(t.autograd.Function):
    """agg[d] = sum_{e: dst(e)=d} val[e] * x[src(e)] on the SpMM kernel; backward on the transposed CSR."""

    @staticmethod
    def forward(ctx, x: Tensor, by_dst: ops.DeviceCSR, by_src: ops.DeviceCSR):
        y = t.empty(by_dst.n_rows, x.shape[1], device=x.device)
        ops.spmm(by_dst, x if x.stride(-1) == 1 else x.contiguous(), Y=y)
        ctx.by_src = by_src
        return y

    @staticmethod
    def backward(ctx, gy: Tensor):
        gx = t.empty(ctx.by_src.n_rows, gy.shape[1], device=gy.device)
        ops.spmm(ctx.by_src, gy.contiguous(), Y=gx)
        return gx, None, None


def block_csr(block: dict) -> Tuple[ops.DeviceCSR, ops.DeviceCSR]:
    """(CSR by destination, CSR by source) of a block with values w / clamp(sum_dst w, min=1).  A block built on the
    device (PinSAGESampler._sample_batch_device) brings both with it."""
    if "csr" in block:
        return block["csr"]
    n_src, n_dst = block["src_ids"].numel(), block["n_dst"]
    es, ed, w = block["edge_src"].contiguous(), block["edge_dst"].contiguous(), block["weights"].contiguous()
    ws = t.zeros(n_dst, device=w.device).index_add_(0, ed, w).clamp(min=1)
    val = w / ws[ed]
    by_dst = ops.coo_to_csr(ed, es, n_dst, n_src)
    by_dst.val = ops.gather_f32(val, by_dst.perm) if val.numel() else val
    by_src = ops.coo_to_csr(es, ed, n_src, n_dst)
    by_src.val = ops.gather_f32(val, by_src.perm) if val.numel() else val
    return by_dst, by_src


class WeightedSAGEConv(nn.Module):
    def __init__(self, input_dims: int, hidden_dims: int, output_dims: int):
        super().__init__()
        self.Q = Linear(input_dims, hidden_dims)
        self.W = Linear(input_dims + hidden_dims, output_dims)
        self.dropout = nn.Dropout(0.5)
        self.reset_parameters()

    def reset_parameters(self) -> None:
        gain = nn.init.calculate_gain("relu")
        nn.init.xavier_uniform_(self.Q.weight, gain=gain)
        nn.init.xavier_uniform_(self.W.weight, gain=gain)
        nn.init.constant_(self.Q.bias, 0)
        nn.init.constant_(self.W.bias, 0)

    def forward(self, block: dict, h_src: Tensor, h_dst: Tensor) -> Tensor:
        n = self.Q(self.dropout(h_src), relu=True)
        by_dst, by_src = block_csr(block)
        agg = _WeightedSumFn.apply(n, by_dst, by_src)          # = (sum_e w n_src) / clamp(sum_e w, 1)
        z = self.W(self.dropout(t.cat([agg, h_dst], 1)), relu=True)
        z_norm = z.norm(2, 1, keepdim=True)
        z_norm = t.where(z_norm == 0, t.ones_like(z_norm), z_norm)
        return z / z_norm


class PinSAGEModel(nn.Module):
    def __init__(self, n_items: int, hidden_dims: int, n_layers: int, features: Optional[ItemFeatures] = None,
                 use_id: bool = True, sparse_tables: bool = False):
        """features=None, use_id=True: the id-only model (the id is the one feature the reference's dataset assigns).  With
        `features` the LinearProjector sums the id row (if use_id) with every feature column's projection (ItemProjector):
        an item without interactions, whose id row is never trained, is then placed by its features.
        sparse_tables=True (the reference's pinsage/model_sparse.py: nn.Embedding(sparse=True) + SparseAdam): the id table and
        every text table are LAZY — trained by torch.optim.SparseAdam(model.sparse_parameters()) beside
        torch.optim.Adam(model.dense_parameters()); only the rows a batch references move, and a step costs what the batch
        costs, not what the tables do.  Parameter names, order and initial draws are the same either way."""
        super().__init__()
        self.sparse_tables = bool(sparse_tables)
        if features is None and not use_id:
            raise ValueError("PinSAGEModel: use_id=False needs features (nothing would be projected)")
        if features is not None and features.n_items != n_items:
            raise ValueError(f"PinSAGEModel: features describe {features.n_items} items, the model {n_items}")
        self.n_items, self.hidden = int(n_items), int(hidden_dims)
        if use_id:
            self.proj = nn.Embedding(n_items + 1, hidden_dims)     # LinearProjector over the `id` feature
            nn.init.xavier_uniform_(self.proj.weight)
        self.convs = nn.ModuleList([WeightedSAGEConv(hidden_dims, hidden_dims, hidden_dims) for _ in range(n_layers)])
        self.bias = nn.Parameter(t.zeros(n_items, 1))          # ItemToItemScorer
        if features is not None:
            self.projector = ItemProjector(features, hidden_dims, self.proj if use_id else None)
            self.projector.sparse_tables = self.sparse_tables

    @property
    def featured(self) -> bool:
        return hasattr(self, "projector")

    def sparse_parameters(self) -> List[nn.Parameter]:
        """The lazy tables, in parameters() order: the id table and the text tables of a sparse_tables model; else nothing."""
        if not self.sparse_tables:
            return []
        out = [self.proj.weight] if hasattr(self, "proj") else []
        if self.featured and self.projector.n_text:
            out += list(self.projector.text_tables)
        return out

    def dense_parameters(self) -> List[nn.Parameter]:
        """parameters() without sparse_parameters(), in the same order."""
        lazy = {id(p) for p in self.sparse_parameters()}
        return [p for p in self.parameters() if id(p) not in lazy]

    def project(self, ids: Tensor) -> Tensor:
        """LinearProjector over the rows `ids`: the id table alone, or the feature projector."""
        if self.featured:
            return self.projector(ids)
        return _EmbedRowsFn.apply(self.proj.weight, ids, self.sparse_tables)

    def get_repr(self, blocks: List[dict]) -> Tensor:
        h = self.project(blocks[0]["src_ids"])
        last = blocks[-1]
        h_dst_final = self.project(last["src_ids"][: last["n_dst"]])
        for conv, block in zip(self.convs, blocks):
            h = conv(block, h, h[: block["n_dst"]])
        return h_dst_final + h

    def item_representations(self, sampler, *, step: Optional[int] = None) -> Tensor:
        """The representation of every item, [n_items, hidden] — the evaluation half of pinsage/model.py:120-134 (get_repr
        over collate_test's blocks for batches of item ids), in eval mode with no autograd; the module's train / eval mode
        is restored afterwards.  `step` (default sampler.step) keys the walks with sampler.seed: the same (seed, step)
        gives the same bits on every call.

        One native call (mi_pinsage_embed_items_f32: a layer-by-layer pass over the catalogue, every item's neighbours
        sampled once per layer) where the kernel takes the shapes; otherwise the reference-shaped path, sample_blocks +
        get_repr over batches of sampler.batch_size item ids.  The two agree to rounding (DESIGN §7, N5 evaluation)."""
        from .native import embed_items
        step = int(sampler.step if step is None else step)
        was_training = self.training
        self.eval()
        try:
            with t.no_grad():
                h = embed_items(self, sampler, step)
                if h is None:
                    h = self.batched_item_representations(sampler, step)
        finally:
            self.train(was_training)
        return h

    def batched_item_representations(self, sampler, step: int, batch_size: Optional[int] = None) -> Tensor:
        """get_repr over sample_blocks(batch, step) for consecutive batches of item ids (pinsage/sampler.py:181-185), as the
        reference evaluates; the caller sets eval mode and no_grad (item_representations does)."""
        ids = t.arange(self.n_items, device=self.bias.device)
        return t.cat([self.get_repr(sampler.sample_blocks(b, step))
                      for b in ids.split(int(batch_size or sampler.batch_size))], 0)

    def score(self, h: Tensor, seeds: Tensor, pair) -> Tensor:
        u, v = pair
        return (h[u] * h[v]).sum(1, keepdim=True) + self.bias[seeds[u]] + self.bias[seeds[v]]

    def forward(self, seeds: Tensor, pos, neg, blocks: List[dict]) -> Tensor:
        h = self.get_repr(blocks)
        return (self.score(h, seeds, neg) - self.score(h, seeds, pos) + 1).clamp(min=0)


def train_epoch(model: PinSAGEModel, optimizer: t.optim.Optimizer, sampler, batches: int, group=None,
                sparse_optimizer: Optional[t.optim.Optimizer] = None) -> List[float]:
    """pinsage/model.py:118-131: hinge loss mean over the batch's pairs, Adam.  A sparse_tables model (pinsage/model_sparse.py)
    brings its pair: optimizer = Adam(model.dense_parameters()), sparse_optimizer = SparseAdam(model.sparse_parameters()); the
    autograd fallback zeroes and steps both.  Single-process only: a multi-rank run with a sparse optimizer raises.

    Under torch.distributed (BASELINE configs[4]: 4 GPUs) the run is data-parallel: every rank owns a replica and a
    sampler with its own seed (the item-item walks need the whole graph, 0.4 GB of int32 CSR, so it is replicated),
    and the gradients — dense layers plus the id-embedding table — are averaged with one flat all-reduce per
    step (dist_ranker.allreduce_gradients; a no-op when not initialised)."""
    import torch.distributed as dist
    from ..dist_ranker import allreduce_gradients
    from .native import NativePinSAGEStep
    losses = []
    model.train()
    # one C call per iteration where the model / optimizer are the executor's.  Data-parallel: the executor's compact-row mode
    # (the ranks exchange the batch's gradient rows, not the dense 27 MB table gradient) when the sampler's bounds are known;
    # every rank must take the same path, which it does: the choice depends on the model, the optimizer and the sampler's
    # configuration only.
    multi = dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1
    if multi and sparse_optimizer is not None:
        raise ValueError("train_epoch: data-parallel training with a sparse optimizer is not built (the lazy tables' rows would "
                         "have to be exchanged and summed across ranks before the update)")
    if getattr(model, "sparse_tables", False) and sparse_optimizer is None and model.sparse_parameters():
        raise ValueError("train_epoch: a sparse_tables model needs sparse_optimizer (torch.optim.SparseAdam over "
                         "model.sparse_parameters()); its lazy tables' gradients are sparse tensors")
    native = None
    if NativePinSAGEStep.supports(model, optimizer, sparse_optimizer):
        if not multi:
            native = NativePinSAGEStep(model, optimizer, sparse_optimizer)
        elif model.featured:
            native = None    # data-parallel native features are not built: the autograd iteration with its dense all-reduce, on every rank
        elif all(hasattr(sampler, a) for a in ("batch_size", "T", "n_layers")):
            native = NativePinSAGEStep(model, optimizer, data_parallel=True, group=group,
                                       seed=(t.initial_seed() + dist.get_rank(group)) & ((1 << 63) - 1))
            native.exchange_capacity = (3 * sampler.batch_size * (1 + sampler.T) ** sampler.n_layers, 3 * sampler.batch_size)
    # the backward graph is a chain of small nodes: running it in the calling thread saves the hand-over to autograd's
    # device thread at every one of them (as training.train_with_dataloader does for the ranker); the losses are read
    # back once per epoch, not once per step
    with t.autograd.set_multithreading_enabled(False):
        # sampler.batches: batch i + 1 is drawn on a side stream while this loop trains on batch i
        source = sampler.batches(batches) if hasattr(sampler, "batches") else (sampler.sample_batch() for _ in range(batches))
        for b in source:
            loss = native.step(b) if native is not None else None
            if loss is not None:
                losses.append(loss[0])
                continue
            # a declined batch: in a data-parallel run the executor's decline is collective (one all-reduce(MIN) of a flag before
            # anything is enqueued, pinsage/native.py), so EVERY rank is here with its own batch and the autograd iteration
            # below — with its dense all-reduce — runs on all of them
            loss = model(b["seeds"], b["pos"], b["neg"], b["blocks"]).mean()
            optimizer.zero_grad()
            if sparse_optimizer is not None:
                sparse_optimizer.zero_grad()
            loss.backward()
            allreduce_gradients(model.parameters(), group)
            optimizer.step()
            if sparse_optimizer is not None:
                sparse_optimizer.step()
            losses.append(loss.detach())
    return t.stack(losses).cpu().tolist() if losses else []
