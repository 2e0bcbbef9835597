"""One PinSAGE training iteration as one C call (mi_pinsage_step_f32, csrc/pinsage_exec.hip) — the loop body of the
reference's pinsage/model.py:118-131 on PinSAGEModel (pinsage/model.py:16-34, pinsage/layers.py:121-203).

The model, its parameters and the optimizer stay torch's own: gradients land in `param.grad`, Adam's moments in
`optimizer.state[p]`.  Two dense gradient buffers (the projector table's and the scorer bias's) are kept all-zero between
iterations by the executor itself: it writes the rows of the batch, runs torch.optim.Adam's dense update over the whole
tables and clears the rows again, so after a step those two `.grad`s read zero (keep_grads=True stops after the gradients
and leaves them in place instead).  Batches must come from PinSAGESampler (its block layout: destination nodes first; the
index-op path's blocks get their CSRs built here); a model / optimizer / batch outside the executor's shapes is declined
and the caller takes the autograd path (pinsage.model.train_epoch does that by itself).

A model with item features (PinSAGEModel(features=...)) runs the same executor between the projector's two calls: the rows of
blocks[0].src_ids — distinct, and holding every block's destination nodes — are projected into a compact table
(mi_pinsage_project_f32), the executor runs on it with apply_adam = 0 and hands the gradient of those rows back compactly
(rows_out / bias_out), mi_pinsage_project_bwd_f32 turns it into the tables', the id table's and the Linear's gradients, and
mi_adam_multi_f32 applies torch.optim.Adam's dense update to every tensor; the table rows written are cleared again
(mi_pinsage_project_clear_f32), so the table gradients stay all-zero between iterations as the id table's does.  Text columns
(ItemFeatures(text=...)) are one more pair of calls beside those: mi_pinsage_text_f32 after the projector's forward (accumulating
into its rows; alone for a text-only model), mi_pinsage_text_bwd_f32 after its backward, mi_pinsage_text_clear_f32 after its
clear; the text tables are ordinary entries of mi_adam_multi_f32's list.  All of those calls are ItemProjector's own methods
(project / project_backward / clear_rows, pinsage/model.py) over its cached descriptors and workspaces: the step only says when.

The sparse trainer (PinSAGEModel(sparse_tables=True) with its pair of optimizers, the reference's pinsage/model_sparse.py): the id
table and the text tables are LAZY — torch.optim.SparseAdam's update on the rows the batch references and nothing else.  Both model
kinds then run the executor in rows_out mode with apply_adam = 0; the id-only model hands the compact rows of blocks[0].src_ids
(distinct) to mi_lazy_adam_rows_f32, a featured model takes mi_pinsage_project_bwd_lazy_f32 / mi_pinsage_text_bwd_lazy_f32 in place
of the two backwards; then the scorer-bias scatter, mi_adam_multi_f32 over the DENSE set only, and the clear.  Nothing in the
iteration walks a lazy table: `p.grad` of a lazy table stays None (the id-only model has no table-sized gradient at all; a
featured model's summed rows pass through a zero-kept buffer the step owns), and sparse_optimizer.state[p] keeps torch's layout
(`step` a Python int, dense exp_avg / exp_avg_sq), so its state_dict() loads into a fresh SparseAdam and the reverse.

The host side shared with the ranker's executor — Adam's state, the flat gradient buffer, the workspace growth rule, the
stale-descriptor test, the collective decline — is native_binding.py.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import torch as t
from torch import Tensor

from .. import _lib
from .._lib import PinsageModel, PinsageStepBatch
from ..model.layers import _ones4
from ..native_binding import (PEER_DECLINED, PointerSnapshot, adam_unsupported_reason, all_ranks_take_it, bind_param,
                              bump_adam_steps, collective_prepare, ensure_adam_state, flat_grad_views, grown_workspace)
from .model import PinSAGEModel


def _conv_params(cv):
    return cv.Q.weight, cv.Q.bias, cv.W.weight, cv.W.bias


def _fill_convs(d: PinsageModel, model: PinSAGEModel, with_grads: bool) -> None:
    for l, cv in enumerate(model.convs):
        c = d.conv[l]
        c.q_w, c.q_b, c.w_w, c.w_b = (x.data_ptr() for x in _conv_params(cv))
        if with_grads:
            c.g_q_w, c.g_q_b, c.g_w_w, c.g_w_b = (x.grad.data_ptr() for x in _conv_params(cv))


class NativePinSAGEStep:
    def __init__(self, model: PinSAGEModel, optimizer: t.optim.Optimizer, sparse_optimizer: Optional[t.optim.Optimizer] = None,
                 seed: Optional[int] = None, keep_grads: bool = False, data_parallel: bool = False, group=None):
        """data_parallel (BASELINE configs[4]: 4 GPUs): every rank runs the executor on its own batch with the projector / bias
        gradients written COMPACTLY (the rows of the batch), the ranks all-gather those lists (a few hundred KB instead of an
        all-reduce of the dense 27 MB table gradient), all-reduce the dense layers' gradients (one flat buffer), and
        mi_pinsage_apply_f32 adds every rank's rows in rank order, applies Adam on the mean gradient and clears the rows:
        replicas stay bitwise identical.  Batches must keep the sampler's size bounds (they size the exchange buffer)."""
        if data_parallel and sparse_optimizer is not None:
            raise ValueError("NativePinSAGEStep: data_parallel with a sparse optimizer is not built (the lazy tables' rows of every "
                             "rank would have to be exchanged and summed before the update)")
        if data_parallel and getattr(model, "featured", False):
            raise ValueError("NativePinSAGEStep: data_parallel with item features is not built (the compact row exchange carries "
                             "id-table rows only); use the autograd iteration with its dense all-reduce")
        why = self.unsupported_reason(model, optimizer, sparse_optimizer)
        if why:
            raise ValueError(f"NativePinSAGEStep: {why}")
        if data_parallel and keep_grads:
            raise ValueError("NativePinSAGEStep: keep_grads is a single-process probe")
        self.model, self.optimizer, self.keep_grads = model, optimizer, bool(keep_grads)
        self.sparse_optimizer = sparse_optimizer
        self._lazy: list = model.sparse_parameters() if sparse_optimizer is not None else []
        self._lazy_g: dict = {}                        # featured: lazy table -> the zero-kept buffer its summed rows pass through
        self._kept_ids: Optional[Tensor] = None        # keep_grads: blocks[0].src_ids of the last step (table_grad)
        self.data_parallel, self.group = bool(data_parallel), group
        self._flat_small: Optional[Tensor] = None     # data-parallel: the dense layers' gradients, one allocation
        self._xbuf = None                              # data-parallel: (send int32 buffer, gathered buffer, capacity in rows)
        self.build_csrs = True     # blocks that come without their CSRs (the sampler's index-op path) get them here
        self.seed = int(t.initial_seed() if seed is None else seed) & ((1 << 64) - 1)
        self.iteration = 0
        self._desc: Optional[PinsageModel] = None
        self._snapshot = None      # native_binding.PointerSnapshot of what _desc was built from
        self._keep: list = []
        self._ws: Optional[Tensor] = None
        self._adam_step = 0
        self.declined: Optional[str] = None
        self._rows: Optional[Tensor] = None            # featured: projected rows / their gradient / bias_out, grown on demand
        self._arange: Optional[Tensor] = None

    # ------------------------------------------------------------------------------------------
    @staticmethod
    def unsupported_reason(model, optimizer, sparse_optimizer=None) -> Optional[str]:
        if not isinstance(model, PinSAGEModel):
            return "not a PinSAGEModel"
        why = adam_unsupported_reason(optimizer)
        if why:
            return why
        g = optimizer.param_groups[0]
        params = list(model.parameters())
        lazy = model.sparse_parameters()
        same = lambda have, want: len(have) == len(want) and all(a is b for a, b in zip(have, want))
        if lazy:
            if sparse_optimizer is None:
                return "a sparse_tables model needs sparse_optimizer: torch.optim.SparseAdam over model.sparse_parameters()"
            if type(sparse_optimizer) is not t.optim.SparseAdam or len(sparse_optimizer.param_groups) != 1:
                return "sparse_optimizer other than a single-group torch.optim.SparseAdam"
            if sparse_optimizer.param_groups[0].get("maximize"):
                return "SparseAdam option maximize"
            if not same(sparse_optimizer.param_groups[0]["params"], lazy):
                return "sparse_optimizer's parameter list is not model.sparse_parameters()"
            if not same(g["params"], model.dense_parameters()):
                return "the optimizer's parameter list is not model.dense_parameters()"
        else:
            if sparse_optimizer is not None:
                return "sparse_optimizer given, but the model has no lazy tables (PinSAGEModel(sparse_tables=True))"
            if not same(g["params"], params):
                return "the optimizer's parameter list is not model.parameters()"
        hidden = model.hidden
        if hidden % 4 or hidden > 128 or not (1 <= len(model.convs) <= _lib.MI_PINSAGE_MAX_LAYERS):
            return "hidden size / layer count outside the executor's"
        if (4 * len(model.convs) if (model.featured or lazy) else len(params) - 1) > _lib.MI_PINSAGE_MAX_PARAMS:
            return "too many parameter tensors"
        if model.featured and model.projector.n_items != model.n_items:
            return "features and model disagree on the item count"
        for cv in model.convs:
            if tuple(cv.Q.weight.shape) != (hidden, hidden) or tuple(cv.W.weight.shape) != (hidden, 2 * hidden):
                return "layer widths differ from the hidden size"
            if cv.Q.bias is None or cv.W.bias is None:
                return "a layer without bias"
            if cv.dropout.p != model.convs[0].dropout.p:
                return "layers with different dropout rates"
        if any(p.dtype != t.float32 or not p.is_cuda or not p.is_contiguous() or not p.requires_grad for p in params):
            return "parameters are not contiguous float32 CUDA tensors with requires_grad"
        return None

    @classmethod
    def supports(cls, model, optimizer, sparse_optimizer=None) -> bool:
        return cls.unsupported_reason(model, optimizer, sparse_optimizer) is None

    # ------------------------------------------------------------------------------------------
    def _build(self) -> PinsageModel:
        """The executor's descriptor.  Id-only: the id table with its gradient and moments apart (proj / g_proj / m_proj / v_proj),
        every other tensor in `params`.  Featured: over a COMPACT projected table (set per batch, _prepare) — its params are the
        layers' only, it never applies Adam and never touches g_proj / m_proj / v_proj (rows_out mode); every tensor of the
        optimizer's group is in mi_adam_multi_f32's flat list instead.  With lazy tables (sparse trainer) the id-only model takes
        the featured layout too — rows_out mode over the REAL id table, the dense group in the flat list — and the lazy tables get
        torch.optim.SparseAdam's state as that optimizer creates it on its first step."""
        model, opt = self.model, self.optimizer
        lazy = self._lazy
        for p in lazy:
            st = self.sparse_optimizer.state[p]
            if len(st) == 0:
                st["step"] = 0
                st["exp_avg"] = t.zeros_like(p, memory_format=t.preserve_format)
                st["exp_avg_sq"] = t.zeros_like(p, memory_format=t.preserve_format)
        d = PinsageModel()
        keep = self._keep = []
        group = opt.param_groups[0]
        params = group["params"]
        if self.data_parallel:   # every gradient except the two dense tables': views of one flat buffer (one all-reduce)
            small = [p for p in params if p is not model.proj.weight and p is not model.bias]
            self._flat_small = flat_grad_views(small, self._flat_small, keep_values=False)
            keep.append(self._flat_small)
        for p in params:
            if p.grad is None or p.grad.shape != p.shape or not p.grad.is_contiguous():
                p.grad = t.zeros_like(p)
            st = ensure_adam_state(opt, group, p)
            keep += [p.grad, st["exp_avg"], st["exp_avg_sq"]]
        bias, pr = model.bias, (model.projector if model.featured else None)
        # the dense buffers kept all-zero between iterations: the scorer bias's and every table's (id and text tables included)
        tables = [model.proj.weight] if pr is None else [p for p in pr.parameter_list() if p is not pr.weight and p is not pr.bias]
        if pr is not None:
            for p in lazy:
                have = self._lazy_g.get(p)
                if have is None or have.shape != p.shape or have.device != p.device:
                    self._lazy_g[p] = t.empty_like(p, memory_format=t.contiguous_format)
            keep += list(self._lazy_g.values())
        for p in tables + [bias]:
            buf = self._grad_buffer(p)
            if buf is not None:
                buf.zero_()
        d.n_layers, d.hidden, d.n_items = len(model.convs), model.hidden, model.n_items
        d.bias, d.g_bias = bias.data_ptr(), bias.grad.data_ptr()
        _fill_convs(d, model, with_grads=True)
        if pr is None:
            proj = model.proj.weight
            d.hidden, d.n_items = int(proj.shape[1]), int(bias.shape[0])
            if proj.shape[0] != d.n_items + 1:
                raise ValueError("NativePinSAGEStep: projector table and scorer bias disagree on the item count")
            sp = self.sparse_optimizer.state[proj] if lazy else opt.state[proj]
            # lazy: rows_out mode never touches g / m / v (there is no table-sized gradient): any valid address stands in for g
            d.proj, d.g_proj = proj.data_ptr(), (sp["exp_avg"] if lazy else proj.grad).data_ptr()
            d.m_proj, d.v_proj = sp["exp_avg"].data_ptr(), sp["exp_avg_sq"].data_ptr()
            mine = [p for p in params if p is not proj]
            if lazy:
                mine = [p for cv in model.convs for p in _conv_params(cv)]
                self._flat_params = (_lib.RankerParam * len(params))()
                for q, p in zip(self._flat_params, params):
                    bind_param(q, p, p.grad, opt.state[p])
        else:
            mine = [p for cv in model.convs for p in _conv_params(cv)]
            self._flat_params = (_lib.RankerParam * len(params))()
            for q, p in zip(self._flat_params, params):
                bind_param(q, p, p.grad, opt.state[p])
            # the projector's descriptors, checked here and not again until this descriptor is rebuilt (_snapshot_now covers the
            # same tensors); the gradient buffers as one tuple, which the projector recognises by identity
            self._proj_bound, self._proj_grads = pr.bind(), tuple(self._grad_buffer(p) for p in pr.parameter_list())
            sst = self.sparse_optimizer.state if lazy else None
            self._proj_moments = [(sst[p]["exp_avg"], sst[p]["exp_avg_sq"]) if any(p is q for q in lazy) else None
                                  for p in pr.parameter_list()]
        for q, p in zip(d.params, mine):
            bind_param(q, p, p.grad, opt.state[p])
        d.n_params = len(mine)
        self._adam_step = int(opt.state[params[0]]["step"]) if params else 0
        return d

    def _grad_buffer(self, p: Tensor) -> Optional[Tensor]:
        """Where p's gradient lands: p.grad, or for a lazy table the step's own zero-kept buffer (featured) / nothing (id-only)."""
        if any(p is q for q in self._lazy):
            return self._lazy_g.get(p)
        return p.grad

    def _lazy_tensors(self) -> list:
        """The lazy tables with their moments (KeyError when a state was dropped: the snapshot then reads as stale)."""
        st = self.sparse_optimizer.state
        return [x for p in self._lazy for x in (p, st[p]["exp_avg"], st[p]["exp_avg_sq"])]

    def _snapshot_now(self) -> PointerSnapshot:
        """Every tensor of the optimizer's group with its gradient and moments; featured: the projector's data buffers too; the
        lazy tables and their moments."""
        getters = [self.model.projector.feature_buffers] if self.model.featured else []
        if self._lazy:
            getters.append(self._lazy_tensors)
        return PointerSnapshot(getters, optimizer=self.optimizer)

    def _lazy_args(self, params) -> "_lib.LazyAdam":
        """torch.optim.SparseAdam's hyper-parameters and the step of THIS update for `params` (which share their step count)."""
        g, st = self.sparse_optimizer.param_groups[0], self.sparse_optimizer.state
        z = _lib.LazyAdam()
        z.lr, (z.beta1, z.beta2), z.eps = float(g["lr"]), (float(b) for b in g["betas"]), float(g["eps"])
        z.step = int(st[params[0]]["step"]) + 1 if params else 1
        return z

    def table_grad(self, p: Tensor) -> Tensor:
        """keep_grads=True: the gradient of lazy table `p` from the last step — the summed rows of the rows the batch referenced —
        as a coalesced torch.sparse_coo_tensor (what the autograd path's p.grad holds, coalesced).  torch ops: a probe."""
        if not self.keep_grads or self._kept_ids is None or not any(p is q for q in self._lazy):
            raise ValueError("NativePinSAGEStep.table_grad: needs keep_grads=True, a step taken, and a lazy table of the model")
        ids0 = self._kept_ids
        if not self.model.featured:
            return t.sparse_coo_tensor(ids0.reshape(1, -1), self._rows[1][: ids0.numel()].clone(), tuple(p.shape)).coalesce()
        pr = self.model.projector
        k = [i for i, q in enumerate(pr.parameter_list()) if q is p][0]
        rows = pr.referenced_rows(ids0)[k]
        return t.sparse_coo_tensor(rows.reshape(1, -1), self._lazy_g[p][rows], tuple(p.shape)).coalesce()

    # ------------------------------------------------------------------------------------------
    def _prepare(self, batch: dict):
        """Everything up to (not including) the launch, the executor's own validation pass included (mi_pinsage_step_check).
        Returns (d, b, loss, keep-alive) or None with self.declined set; nothing has been enqueued either way."""
        model = self.model
        if not model.training:
            self.declined = "model in eval mode"
            return None
        blocks = batch["blocks"]
        if len(blocks) != len(model.convs):
            self.declined = "as many blocks as layers expected"
            return None
        if any("csr" not in b for b in blocks):
            if not self.build_csrs:
                self.declined = "blocks without their CSRs (not a device-built batch)"
                return None
            from .model import block_csr           # index-op batches (sizes beyond the device builder's): two sorts per block
            for b in blocks:
                if "csr" not in b:
                    b["csr"] = block_csr(b)
        seeds, (pu, pv), (nu, nv) = batch["seeds"], batch["pos"], batch["neg"]
        if pu.numel() == 0 or nu.data_ptr() != pu.data_ptr():
            self.declined = "no pairs / negative pairs with their own heads"
            return None
        if self._desc is None or not self._snapshot.current():
            self._desc = self._build()
            self._snapshot = self._snapshot_now()
        elif self.keep_grads:      # the previous call left its rows in the dense buffers
            for p in ([model.bias] + model.projector.parameter_list()) if model.featured else (model.proj.weight, model.bias):
                buf = self._grad_buffer(p)
                if buf is not None:
                    buf.zero_()
        if self._lazy:
            idw = model.proj.weight if hasattr(model, "proj") else None
            steps = {int(self.sparse_optimizer.state[p]["step"]) for p in self._lazy if p is not idw}
            if len(steps) > 1:
                self.declined = "text tables with different SparseAdam step counts"
                return None
        d = self._desc
        group = self.optimizer.param_groups[0]
        d.p_dropout = float(model.convs[0].dropout.p)
        d.lr, (d.beta1, d.beta2), d.eps = float(group["lr"]), (float(b) for b in group["betas"]), float(group["eps"])
        d.apply_adam = 0 if (self.keep_grads or self.data_parallel or model.featured or self._lazy) else 1
        d.step = self._adam_step + 1
        b = PinsageStepBatch()
        b.n_blocks = len(blocks)
        keep = []
        for l, blk in enumerate(blocks):
            by_dst, by_src = blk["csr"]
            sb = b.blocks[l]
            sb.n_src, sb.n_dst, sb.nnz = int(blk["src_ids"].numel()), int(blk["n_dst"]), int(by_dst.nnz)
            sb.src_ids = blk["src_ids"].data_ptr()
            sb.dst_rowptr, sb.src_rowptr = by_dst.rowptr.data_ptr(), by_src.rowptr.data_ptr()
            if by_dst.nnz:
                sb.dst_col, sb.dst_val = by_dst.col.data_ptr(), by_dst.val.data_ptr()
                sb.src_col, sb.src_val = by_src.col.data_ptr(), by_src.val.data_ptr()
            keep.append((by_dst, by_src))
        b.n_seeds, b.n_pairs = int(seeds.numel()), int(pu.numel())
        b.seeds, b.pos_u, b.pos_v, b.neg_v = seeds.data_ptr(), pu.data_ptr(), pv.data_ptr(), nv.data_ptr()
        b.seed, b.step = self.seed, self.iteration
        loss = t.empty(1, dtype=t.float32, device=seeds.device)
        b.loss = loss.data_ptr()
        ones = _ones4(max(int(blk["src_ids"].numel()) for blk in blocks), seeds.device)
        d.ones4, d.n_ones = ones.data_ptr(), int(ones.shape[0])
        if self.data_parallel:
            send = self._exchange_buffer(b, blocks[0]["src_ids"], seeds)
            if send is None:
                return None
        if model.featured or self._lazy:
            # featured: the executor reads row r of a compact table for block 0's r-th source: its ids are 0 .. n0 - 1.  Lazy
            # id-only: the real table and ids, only the gradient rows come back compactly.
            n0, H = int(blocks[0]["src_ids"].numel()), model.hidden
            if self._rows is None or self._rows.shape[1] < n0:
                cap = max(1024, int(n0 * 1.25))
                self._rows = t.empty(3, cap, H, dtype=t.float32, device=seeds.device)   # projected rows, their gradient, bias_out
                self._arange = t.arange(cap, dtype=t.int64, device=seeds.device)
            rows = self._rows
            if model.featured:
                b.blocks[0].src_ids = self._arange.data_ptr()
                d.proj = d.g_proj = d.m_proj = d.v_proj = rows[0].data_ptr()      # g / m / v: never touched in rows_out mode
            b.rows_out, b.bias_out = rows[1].data_ptr(), rows[2].data_ptr()
        L = _lib.lib()
        need = int(L.mi_pinsage_step_workspace_bytes(ctypes.byref(d), ctypes.byref(b)))
        self._ws = grown_workspace(self._ws, need, seeds.device)
        if self._world() > 1:      # the validation pass on its own only where the ranks must agree before anything is enqueued
            rc = L.mi_pinsage_step_check(ctypes.byref(d), ctypes.byref(b), self._ws.data_ptr(), self._ws.numel())
            if rc == _lib.MI_ERR_UNSUPPORTED:
                self.declined = "mi_pinsage_step_f32: MI_ERR_UNSUPPORTED (shape outside the executor's)"
                self._desc = None      # the caller's own step may leave anything in the gradient buffers: start clean next time
                return None
            _lib.check(rc, "mi_pinsage_step_check")
        return d, b, loss, (keep, ones, seeds, pu, pv, nv)

    def _world(self) -> int:
        import torch.distributed as dist
        return dist.get_world_size(self.group) if (self.data_parallel and dist.is_initialized()) else 1

    def _all_ranks_take_it(self, mine: bool, device) -> bool:
        return all_ranks_take_it(mine, device, self.group)

    def step(self, batch: dict) -> Optional[Tensor]:
        """One iteration on a PinSAGESampler batch; the loss as a 1-element device tensor, or None when declined (nothing
        has been enqueued then).  Data-parallel with more than one rank: the decline is COLLECTIVE (native_binding), so that a rank
        whose batch lies outside the executor's shapes, or whose _prepare raises, does not leave its peers waiting in the row
        exchange; every rank returns None together."""
        self.declined = None
        world = self._world()
        prep, go = collective_prepare(world, lambda mine: self._all_ranks_take_it(mine, self.model.bias.device),
                                      lambda: self._prepare(batch))
        if not go:
            if prep is not None:
                self.declined = PEER_DECLINED
                self._desc = None
            return None
        d, b, loss, _keep = prep
        group = self.optimizer.param_groups[0]
        L = _lib.lib()
        pr = self.model.projector if self.model.featured else None
        lazy = self._lazy
        if pr is not None or lazy:
            ids0, rows = batch["blocks"][0]["src_ids"], self._rows
        if pr is not None:
            bound = self._proj_bound
            pr.project(ids0, out=rows[0], bound=bound)
        rc = L.mi_pinsage_step_f32(ctypes.byref(d), ctypes.byref(b), self._ws.data_ptr(), self._ws.numel(), _lib.current_stream())
        if rc == _lib.MI_ERR_UNSUPPORTED:
            if world > 1:                      # cannot happen: mi_pinsage_step_check took the same descriptors
                raise _lib.MiError("mi_pinsage_step_f32 declined a batch its own validation pass had accepted")
            self.declined = "mi_pinsage_step_f32: MI_ERR_UNSUPPORTED (shape outside the executor's)"
            self._desc = None      # the caller's own step may leave anything in the gradient buffers: start clean next time
            return None
        _lib.check(rc, "mi_pinsage_step_f32")
        self.iteration += 1
        if self.data_parallel:
            self._exchange_and_apply(d)
        if pr is not None or lazy:
            seeds = batch["seeds"]
            self._kept_ids = ids0 if self.keep_grads else None
            if pr is None:           # lazy id-only: the compact rows of the distinct ids straight into the row update
                if not self.keep_grads:
                    proj, st = self.model.proj.weight, self.sparse_optimizer.state[self.model.proj.weight]
                    ids0 = ids0.contiguous()
                    _lib.check(L.mi_lazy_adam_rows_f32(int(proj.shape[0]), int(proj.shape[1]), proj.data_ptr(), st["exp_avg"].data_ptr(),
                                                       st["exp_avg_sq"].data_ptr(), int(ids0.numel()), ids0.data_ptr(), rows[1].data_ptr(),
                                                       int(rows[1].stride(0)), ctypes.byref(self._lazy_args([proj])),
                                                       _lib.current_stream()), "mi_lazy_adam_rows_f32")
            elif lazy and not self.keep_grads:
                ids_p = [p for p in lazy if p is pr.id_weight]
                text_p = [p for p in lazy if p is not pr.id_weight]
                pr.project_backward_lazy(ids0, rows[1], self._proj_grads, self._proj_moments,
                                         (self._lazy_args(ids_p), self._lazy_args(text_p)), bound=bound)
            else:
                pr.project_backward(ids0, rows[1], self._proj_grads, bound=bound)
            gb = self.model.bias.grad.view(-1)
            gb.index_copy_(0, seeds, rows[2].view(-1)[: seeds.numel()])     # the seeds are distinct
            if not self.keep_grads:
                _lib.check(L.mi_adam_multi_f32(self._flat_params, len(self._flat_params), float(group["lr"]),
                                               float(group["betas"][0]), float(group["betas"][1]), float(group["eps"]),
                                               self._adam_step + 1, _lib.current_stream()), "mi_adam_multi_f32")
                if pr is not None and (not lazy or len(pr.tables)):      # the lazy backward zeroed the lazy tables' rows itself
                    pr.clear_rows(ids0, self._proj_grads, bound=bound, text=not lazy)
                gb.index_fill_(0, seeds, 0.0)
        if not self.keep_grads:
            self._adam_step += 1
            bump_adam_steps([self.optimizer.state[q]["step"] for q in group["params"]])
            for q in lazy:
                self.sparse_optimizer.state[q]["step"] += 1
        return loss

    # ------------------------------------------------------------------------------------------
    # data-parallel exchange.  One int32 buffer per rank: [n_rows, n_seeds, 0, 0 | ids as int64 (2 words each, cap entries) |
    # rows as float32 (cap * hidden) | bias as float32 (cap_seeds)]; the executor writes rows / bias straight into it.
    def _layout(self, hidden: int):
        cap, cap_s = self._xbuf[2], self._xbuf[3]
        o_ids = 4
        o_rows = o_ids + 2 * cap
        o_bias = o_rows + cap * hidden
        return cap, cap_s, o_ids, o_rows, o_bias, o_bias + cap_s

    def _exchange_buffer(self, b: PinsageStepBatch, ids0: Tensor, seeds: Tensor):
        import torch.distributed as dist
        hidden = int(self.model.proj.weight.shape[1])
        n0, ns = int(ids0.numel()), int(seeds.numel())
        if self._xbuf is None:
            # capacity from the sampler's bounds: 3 B seeds, (1 + T) growth per layer — the same on every rank.  Callers with
            # other batch sources set .exchange_capacity = (rows, seeds) before the first step.
            cap = getattr(self, "exchange_capacity", None)
            if cap is None:
                self.declined = "data_parallel needs .exchange_capacity = (max rows of block 0, max seeds), equal on every rank"
                return None
            world = dist.get_world_size(self.group) if dist.is_initialized() else 1
            rows_cap, seeds_cap = (int(cap[0]) + 3) // 4 * 4, (int(cap[1]) + 3) // 4 * 4   # keeps every section 16-byte aligned
            words = 4 + 2 * rows_cap + rows_cap * hidden + seeds_cap
            dev = seeds.device
            self._xbuf = (t.zeros(words, dtype=t.int32, device=dev), t.zeros(world, words, dtype=t.int32, device=dev), rows_cap,
                          seeds_cap, world)
        cap, cap_s, o_ids, o_rows, o_bias, _ = self._layout(hidden)
        if n0 > cap or ns > cap_s:
            self.declined = f"batch larger than the exchange capacity ({n0} rows / {ns} seeds vs {cap} / {cap_s})"
            return None
        send = self._xbuf[0]
        send[0:2] = t.tensor([n0, ns], dtype=t.int32, device=send.device)
        send[o_ids: o_ids + 2 * n0].view(t.int64).copy_(ids0)
        b.rows_out = send.data_ptr() + 4 * o_rows
        b.bias_out = send.data_ptr() + 4 * o_bias
        return send

    def _exchange_and_apply(self, d: PinsageModel) -> None:
        import torch.distributed as dist
        send, gathered, cap, cap_s, world = self._xbuf
        hidden = int(self.model.proj.weight.shape[1])
        _, _, o_ids, o_rows, o_bias, _ = self._layout(hidden)
        if world > 1:
            # the all-gather as an all-reduce(sum) of a [world, words] int32 buffer that is zero outside the rank's own
            # slot (bit patterns + 0 = bit patterns): the payload is tiny (world x 0.4 MB), and gloo's all_gather takes
            # 225 ms for it on this image (tools/probes/gloo_ops.py) where its all_reduce takes 0.3 ms
            gathered.zero_()
            gathered[dist.get_rank(self.group)].copy_(send)
            dist.all_reduce(gathered, op=dist.ReduceOp.SUM, group=self.group)
            dist.all_reduce(self._flat_small, op=dist.ReduceOp.SUM, group=self.group)
        else:
            gathered[0].copy_(send)
        counts = gathered[:, 0:2].cpu().tolist()     # the one read-back of the exchange (2 ints per rank)
        lists = (_lib.PinsageGradList * world)()
        base, stride = gathered.data_ptr(), 4 * gathered.shape[1]
        for r in range(world):
            lists[r].n_rows, lists[r].n_seeds = int(counts[r][0]), int(counts[r][1])
            lists[r].ids = base + r * stride + 4 * o_ids
            lists[r].rows = base + r * stride + 4 * o_rows
            lists[r].bias = base + r * stride + 4 * o_bias
        _lib.check(_lib.lib().mi_pinsage_apply_f32(ctypes.byref(d), lists, world, 1.0 / world, _lib.current_stream()),
                   "mi_pinsage_apply_f32")


# ---- evaluation: every item's representation in one C call ------------------------------------------------------------------
def embed_items(model: PinSAGEModel, sampler, step: int) -> Optional[Tensor]:
    """PinSAGEModel.get_repr of every item, for the sampler's (seed, step), as one mi_pinsage_embed_items_f32 call
    (csrc/pinsage_infer.hip): [n_items, hidden] fp32.  None when the model or the sampler lies outside the kernel's shapes
    (nothing has been enqueued then); the caller takes the batched path.  Eval semantics (no dropout); no autograd."""
    if not isinstance(model, PinSAGEModel) or not all(hasattr(sampler, a) for a in ("iu_ptr", "ui_ptr", "L", "p", "W", "T")):
        return None
    hidden, n_items = model.hidden, model.n_items
    dev = model.bias.device
    params = ([] if model.featured else [model.proj.weight]) + [x for cv in model.convs for x in _conv_params(cv)]
    if (hidden % 4 or hidden > 128 or not (1 <= len(model.convs) <= _lib.MI_PINSAGE_MAX_LAYERS) or sampler.T > 16
            or n_items != sampler.num_items or len(model.convs) != sampler.n_layers):
        return None
    if any(x is None or x.dtype != t.float32 or not x.is_cuda or not x.is_contiguous() or x.device != dev for x in params):
        return None
    for cv in model.convs:
        if tuple(cv.Q.weight.shape) != (hidden, hidden) or tuple(cv.W.weight.shape) != (hidden, 2 * hidden):
            return None
    if sampler.iu_ptr.device != dev:
        return None
    # featured: the whole catalogue projected by one forward call (after every check: a decline enqueues nothing); the kernel
    # reads rows 0 .. n_items - 1 of `proj`
    proj = model.projector.project(None) if model.featured else model.proj.weight
    d = PinsageModel()
    d.n_layers, d.hidden, d.n_items = len(model.convs), hidden, n_items
    d.proj = proj.data_ptr()
    _fill_convs(d, model, with_grads=False)
    L = _lib.lib()
    out = t.empty(n_items, hidden, dtype=t.float32, device=proj.device)
    ws = t.empty(int(L.mi_pinsage_embed_items_workspace_bytes(n_items, hidden, sampler.T)), dtype=t.uint8, device=proj.device)
    rc = L.mi_pinsage_embed_items_f32(ctypes.byref(d), sampler.iu_ptr.data_ptr(), sampler.iu_idx.data_ptr(),
                                      sampler.ui_ptr.data_ptr(), sampler.ui_idx.data_ptr(), sampler.L, sampler.p, sampler.W,
                                      sampler.T, sampler.seed & ((1 << 64) - 1), int(step), out.data_ptr(), ws.data_ptr(),
                                      ws.numel(), _lib.current_stream())
    if rc == _lib.MI_ERR_UNSUPPORTED:
        return None
    _lib.check(rc, "mi_pinsage_embed_items_f32")
    return out
