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
clear; the text tables are ordinary entries of mi_adam_multi_f32's list.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import torch as t
from torch import Tensor

from .. import _lib
from .._lib import PinsageModel, PinsageStepBatch
from ..model.layers import _ones4
from .model import PinSAGEModel


class NativePinSAGEStep:
    def __init__(self, model: PinSAGEModel, optimizer: t.optim.Optimizer, seed: Optional[int] = None, keep_grads: bool = False,
                 data_parallel: bool = False, group=None):
        """data_parallel (BASELINE configs[4]: 4 GPUs): every rank runs the executor on its own batch with the projector / bias
        gradients written COMPACTLY (the rows of the batch), the ranks all-gather those lists (a few hundred KB instead of an
        all-reduce of the dense 27 MB table gradient), all-reduce the dense layers' gradients (one flat buffer), and
        mi_pinsage_apply_f32 adds every rank's rows in rank order, applies Adam on the mean gradient and clears the rows:
        replicas stay bitwise identical.  Batches must keep the sampler's size bounds (they size the exchange buffer)."""
        if data_parallel and getattr(model, "featured", False):
            raise ValueError("NativePinSAGEStep: data_parallel with item features is not built (the compact row exchange carries "
                             "id-table rows only); use the autograd iteration with its dense all-reduce")
        why = self.unsupported_reason(model, optimizer)
        if why:
            raise ValueError(f"NativePinSAGEStep: {why}")
        if data_parallel and keep_grads:
            raise ValueError("NativePinSAGEStep: keep_grads is a single-process probe")
        self.model, self.optimizer, self.keep_grads = model, optimizer, bool(keep_grads)
        self.data_parallel, self.group = bool(data_parallel), group
        self._flat_small: Optional[Tensor] = None     # data-parallel: the dense layers' gradients, one allocation
        self._xbuf = None                              # data-parallel: (send int32 buffer, gathered buffer, capacity in rows)
        self.build_csrs = True     # blocks that come without their CSRs (the sampler's index-op path) get them here
        self.seed = int(t.initial_seed() if seed is None else seed) & ((1 << 64) - 1)
        self.iteration = 0
        self._desc: Optional[PinsageModel] = None
        self._keep: list = []
        self._ws: Optional[Tensor] = None
        self._adam_step = 0
        self.declined: Optional[str] = None
        self._rows: Optional[Tensor] = None            # featured: projected rows / their gradient / bias_out, grown on demand
        self._arange: Optional[Tensor] = None

    # ------------------------------------------------------------------------------------------
    @staticmethod
    def unsupported_reason(model, optimizer) -> Optional[str]:
        if not isinstance(model, PinSAGEModel):
            return "not a PinSAGEModel"
        if type(optimizer) is not t.optim.Adam or len(optimizer.param_groups) != 1:
            return "optimizer is not a single-group torch.optim.Adam"
        g = optimizer.param_groups[0]
        if g.get("amsgrad") or g.get("weight_decay", 0) or g.get("maximize") or g.get("capturable") or g.get("differentiable"):
            return "Adam options (amsgrad / weight_decay / maximize / capturable)"
        params = list(model.parameters())
        if len(g["params"]) != len(params) or any(a is not b for a, b in zip(g["params"], params)):
            return "the optimizer's parameter list is not model.parameters()"
        hidden = model.hidden
        if hidden % 4 or hidden > 128 or not (1 <= len(model.convs) <= _lib.MI_PINSAGE_MAX_LAYERS):
            return "hidden size / layer count outside the executor's"
        if (4 * len(model.convs) if model.featured else len(params) - 1) > _lib.MI_PINSAGE_MAX_PARAMS:
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
    def supports(cls, model, optimizer) -> bool:
        return cls.unsupported_reason(model, optimizer) is None

    # ------------------------------------------------------------------------------------------
    def _build(self) -> PinsageModel:
        model, opt = self.model, self.optimizer
        d = PinsageModel()
        keep = self._keep = []
        group = opt.param_groups[0]
        if self.data_parallel:   # every gradient except the two dense tables': views of one flat buffer (one all-reduce)
            small = [p for p in group["params"] if p is not model.proj.weight and p is not model.bias]
            offs, total = [], 0
            for p in small:
                offs.append(total)
                total += (p.numel() + 3) // 4 * 4
            flat = self._flat_small
            if flat is None or flat.numel() != total or any(
                    p.grad is None or p.grad.data_ptr() != flat.data_ptr() + 4 * o for p, o in zip(small, offs)):
                flat = t.zeros(total, dtype=t.float32, device=model.proj.weight.device)
                for p, o in zip(small, offs):
                    p.grad = flat[o: o + p.numel()].view(p.shape)
                self._flat_small = flat
            keep.append(flat)
        for p in group["params"]:
            if p.grad is None or p.grad.shape != p.shape or not p.grad.is_contiguous():
                p.grad = t.zeros_like(p)
            st = opt.state[p]
            if len(st) == 0:   # created the way torch.optim.Adam creates it on its first step
                on_device = bool(group.get("fused") or group.get("capturable"))
                st["step"] = t.zeros((), dtype=t.float32, device=p.device) if on_device else t.tensor(0.0, dtype=t.float32)
                st["exp_avg"] = t.zeros_like(p, memory_format=t.preserve_format)
                st["exp_avg_sq"] = t.zeros_like(p, memory_format=t.preserve_format)
            keep += [p.grad, st["exp_avg"], st["exp_avg_sq"]]
        bias = model.bias
        if model.featured:
            return self._build_featured(d)
        proj = model.proj.weight
        proj.grad.zero_()      # the two dense buffers the executor keeps all-zero between iterations
        bias.grad.zero_()
        d.n_layers, d.hidden, d.n_items = len(model.convs), int(proj.shape[1]), int(bias.shape[0])
        if proj.shape[0] != d.n_items + 1:
            raise ValueError("NativePinSAGEStep: projector table and scorer bias disagree on the item count")
        sp = opt.state[proj]
        d.proj, d.g_proj, d.m_proj, d.v_proj = proj.data_ptr(), proj.grad.data_ptr(), sp["exp_avg"].data_ptr(), sp["exp_avg_sq"].data_ptr()
        d.bias, d.g_bias = bias.data_ptr(), bias.grad.data_ptr()
        for l, cv in enumerate(model.convs):
            c = d.conv[l]
            c.q_w, c.q_b, c.w_w, c.w_b = (x.data_ptr() for x in (cv.Q.weight, cv.Q.bias, cv.W.weight, cv.W.bias))
            c.g_q_w, c.g_q_b, c.g_w_w, c.g_w_b = (x.grad.data_ptr() for x in (cv.Q.weight, cv.Q.bias, cv.W.weight, cv.W.bias))
        i = 0
        for p in group["params"]:
            if p is proj:
                continue
            st = opt.state[p]
            q = d.params[i]
            q.p, q.g, q.m, q.v, q.n = p.data_ptr(), p.grad.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel()
            i += 1
        d.n_params = i
        steps = [opt.state[p]["step"] for p in group["params"]]
        self._adam_step = int(steps[0]) if steps else 0
        return d

    def _build_featured(self, d: PinsageModel) -> PinsageModel:
        """The executor's descriptor over a COMPACT projected table (set per batch, _prepare): its params are the layers' only,
        it never applies Adam and never touches g_proj / m_proj / v_proj (rows_out mode).  Also the flat parameter list of
        mi_adam_multi_f32: every tensor of the optimizer's group."""
        model, opt = self.model, self.optimizer
        group = opt.param_groups[0]
        pr = model.projector
        for p in pr.parameter_list():
            if p is not pr.weight and p is not pr.bias:
                p.grad.zero_()     # the table gradients (id and text tables included) stay all-zero between iterations
        model.bias.grad.zero_()
        d.n_layers, d.hidden, d.n_items = len(model.convs), model.hidden, model.n_items
        d.bias, d.g_bias = model.bias.data_ptr(), model.bias.grad.data_ptr()
        i = 0
        for l, cv in enumerate(model.convs):
            c = d.conv[l]
            c.q_w, c.q_b, c.w_w, c.w_b = (x.data_ptr() for x in (cv.Q.weight, cv.Q.bias, cv.W.weight, cv.W.bias))
            c.g_q_w, c.g_q_b, c.g_w_w, c.g_w_b = (x.grad.data_ptr() for x in (cv.Q.weight, cv.Q.bias, cv.W.weight, cv.W.bias))
            for p in (cv.Q.weight, cv.Q.bias, cv.W.weight, cv.W.bias):
                st = opt.state[p]
                q = d.params[i]
                q.p, q.g, q.m, q.v, q.n = p.data_ptr(), p.grad.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel()
                i += 1
        d.n_params = i
        flat = (_lib.RankerParam * len(group["params"]))()
        for q, p in zip(flat, group["params"]):
            st = opt.state[p]
            q.p, q.g, q.m, q.v, q.n = p.data_ptr(), p.grad.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel()
        self._flat_params = flat
        self._proj_grads = [p.grad for p in pr.parameter_list()]
        self._pdesc, self._pgrads = pr.descriptor(), pr.grads_descriptor(self._proj_grads)
        self._pws_rows = -1
        if pr.n_text:
            self._tdesc, self._tgrads = pr.text_descriptor(), pr.text_grads(self._proj_grads)
            self._tws_rows = -1
        steps = [opt.state[p]["step"] for p in group["params"]]
        self._adam_step = int(steps[0]) if steps else 0
        return d

    def _proj_workspace(self, n: int, device) -> Tensor:
        if n > getattr(self, "_pws_rows", -1):
            L, pd = _lib.lib(), ctypes.byref(self._pdesc)
            rows = max(1024, int(n * 1.25))
            need = max(int(L.mi_pinsage_project_workspace_bytes(pd, rows)), int(L.mi_pinsage_project_bwd_workspace_bytes(pd, rows)))
            self._pws, self._pws_rows = t.empty(need, dtype=t.uint8, device=device), rows
        return self._pws

    def _text_workspace(self, n: int, device):
        """(workspace, reference bound) for a block of n rows: the bound is the row capacity times the longest bags, grown on
        demand as _rows grows."""
        if n > getattr(self, "_tws_rows", -1):
            rows = max(1024, int(n * 1.25))
            self._tref_max = self.model.projector.text_ref_bound(rows, True)
            need = int(_lib.lib().mi_pinsage_text_bwd_workspace_bytes(ctypes.byref(self._tdesc), rows, self._tref_max))
            self._tws, self._tws_rows = t.empty(need, dtype=t.uint8, device=device), rows
        return self._tws, self._tref_max

    def _current(self, d: PinsageModel) -> bool:
        """The descriptor holds raw pointers: rebuilt when a parameter, gradient or optimizer-state tensor was replaced."""
        group = self.optimizer.param_groups[0]
        if self.model.featured:
            flat = getattr(self, "_flat_params", None)
            if flat is None or len(flat) != len(group["params"]):
                return False
            for q, p in zip(flat, group["params"]):
                st = self.optimizer.state.get(p)
                if p.grad is None or not st or (q.p, q.g, q.m, q.v) != (p.data_ptr(), p.grad.data_ptr(), st["exp_avg"].data_ptr(),
                                                                        st["exp_avg_sq"].data_ptr()):
                    return False
            pr = self.model.projector
            if (self._pdesc.x, self._pdesc.dense) != (pr.x.data_ptr() if pr.x is not None else None,
                                                      pr.dense.data_ptr() if pr.dense is not None else None):
                return False
            for c in range(pr.n_text):
                if (self._tdesc.ptr[c], self._tdesc.tok[c]) != (getattr(pr, f"text_ptr_{c}").data_ptr(),
                                                                getattr(pr, f"text_tok_{c}").data_ptr()):
                    return False
            return True
        proj = self.model.proj.weight
        i = 0
        for p in group["params"]:
            st = self.optimizer.state.get(p)
            if p.grad is None or not st:
                return False
            if p is proj:
                if (d.proj, d.g_proj, d.m_proj, d.v_proj) != (p.data_ptr(), p.grad.data_ptr(), st["exp_avg"].data_ptr(),
                                                              st["exp_avg_sq"].data_ptr()):
                    return False
                continue
            q = d.params[i]
            if (q.p, q.g, q.m, q.v) != (p.data_ptr(), p.grad.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()):
                return False
            i += 1
        return i == d.n_params

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
        if self._desc is None or not self._current(self._desc):
            self._desc = self._build()
        elif self.keep_grads:      # the previous call left its rows in the dense buffers
            for p in ([model.bias] + model.projector.parameter_list()) if model.featured else (model.proj.weight, model.bias):
                p.grad.zero_()
        d = self._desc
        group = self.optimizer.param_groups[0]
        d.p_dropout = float(model.convs[0].dropout.p)
        d.lr, (d.beta1, d.beta2), d.eps = float(group["lr"]), (float(b) for b in group["betas"]), float(group["eps"])
        d.apply_adam = 0 if (self.keep_grads or self.data_parallel or model.featured) else 1
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
        if model.featured:
            # the executor reads row r of a compact table for block 0's r-th source: its ids are 0 .. n0 - 1
            n0, H = int(blocks[0]["src_ids"].numel()), model.hidden
            if self._rows is None or self._rows.shape[1] < n0:
                cap = max(1024, int(n0 * 1.25))
                self._rows = t.empty(3, cap, H, dtype=t.float32, device=seeds.device)   # projected rows, their gradient, bias_out
                self._arange = t.arange(cap, dtype=t.int64, device=seeds.device)
            rows = self._rows
            b.blocks[0].src_ids = self._arange.data_ptr()
            d.proj = d.g_proj = d.m_proj = d.v_proj = rows[0].data_ptr()      # g / m / v: never touched in rows_out mode
            b.rows_out, b.bias_out = rows[1].data_ptr(), rows[2].data_ptr()
        L = _lib.lib()
        need = int(L.mi_pinsage_step_workspace_bytes(ctypes.byref(d), ctypes.byref(b)))
        if self._ws is None or self._ws.numel() < need:
            self._ws = t.empty(int(need * 1.25) + (1 << 20), dtype=t.uint8, device=seeds.device)
        import torch.distributed as dist
        if self.data_parallel and dist.is_initialized() and dist.get_world_size(self.group) > 1:
            # the validation pass on its own only where the ranks must agree before anything is enqueued
            rc = L.mi_pinsage_step_check(ctypes.byref(d), ctypes.byref(b), self._ws.data_ptr(), self._ws.numel())
            if rc == _lib.MI_ERR_UNSUPPORTED:
                self.declined = "mi_pinsage_step_f32: MI_ERR_UNSUPPORTED (shape outside the executor's)"
                self._desc = None      # the caller's own step may leave anything in the gradient buffers: start clean next time
                return None
            _lib.check(rc, "mi_pinsage_step_check")
        return d, b, loss, (keep, ones, seeds, pu, pv, nv)

    def step(self, batch: dict) -> Optional[Tensor]:
        """One iteration on a PinSAGESampler batch; the loss as a 1-element device tensor, or None when declined (nothing
        has been enqueued then).  Data-parallel with more than one rank: the decline is COLLECTIVE — one all-reduce(MIN) of
        a 1-int flag before anything is enqueued, so that a rank whose batch lies outside the executor's shapes does not
        leave its peers waiting in the row exchange; every rank returns None together."""
        import torch.distributed as dist
        self.declined = None
        prep = self._prepare(batch)
        world = dist.get_world_size(self.group) if (self.data_parallel and dist.is_initialized()) else 1
        if world > 1:
            flag = t.tensor([1 if prep is not None else 0], dtype=t.int32, device=self.model.proj.weight.device)
            dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=self.group)
            if not int(flag.item()):
                if prep is not None:
                    self.declined = "a peer rank declined its batch (collective decision: every rank takes the fallback)"
                    self._desc = None
                return None
        elif prep is None:
            return None
        d, b, loss, _keep = prep
        group = self.optimizer.param_groups[0]
        L = _lib.lib()
        featured = self.model.featured
        if featured:
            # the cached descriptors (rebuilt with the executor's, _current): no per-call ctypes fill on this path
            ids0 = batch["blocks"][0]["src_ids"]
            n0, H = int(ids0.numel()), self.model.hidden
            pr = self.model.projector
            base, text = pr.has_base, pr.n_text > 0
            if base:
                pd, pg, pws = ctypes.byref(self._pdesc), ctypes.byref(self._pgrads), self._proj_workspace(n0, ids0.device)
                _lib.check(L.mi_pinsage_project_f32(pd, n0, ids0.data_ptr(), self._rows[0].data_ptr(), H, pws.data_ptr(), pws.numel(),
                                                    _lib.current_stream()), "mi_pinsage_project_f32")
            if text:
                td, (tws, tref_max) = ctypes.byref(self._tdesc), self._text_workspace(n0, ids0.device)
                _lib.check(L.mi_pinsage_text_f32(td, n0, ids0.data_ptr(), self._rows[0].data_ptr(), H, 1 if base else 0,
                                                 _lib.current_stream()), "mi_pinsage_text_f32")
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
        if featured:
            seeds = batch["seeds"]
            if base:
                _lib.check(L.mi_pinsage_project_bwd_f32(pd, pg, n0, ids0.data_ptr(), self._rows[1].data_ptr(), H, pws.data_ptr(),
                                                        pws.numel(), _lib.current_stream()), "mi_pinsage_project_bwd_f32")
            if text:
                _lib.check(L.mi_pinsage_text_bwd_f32(td, self._tgrads, n0, ids0.data_ptr(), self._rows[1].data_ptr(), H, tref_max,
                                                     tws.data_ptr(), tws.numel(), _lib.current_stream()), "mi_pinsage_text_bwd_f32")
            gb = self.model.bias.grad.view(-1)
            gb.index_copy_(0, seeds, self._rows[2].view(-1)[: seeds.numel()])     # the seeds are distinct
            if not self.keep_grads:
                _lib.check(L.mi_adam_multi_f32(self._flat_params, len(self._flat_params), float(group["lr"]),
                                               float(group["betas"][0]), float(group["betas"][1]), float(group["eps"]),
                                               self._adam_step + 1, _lib.current_stream()), "mi_adam_multi_f32")
                if base:
                    _lib.check(L.mi_pinsage_project_clear_f32(pd, pg, n0, ids0.data_ptr(), _lib.current_stream()),
                               "mi_pinsage_project_clear_f32")
                if text:
                    _lib.check(L.mi_pinsage_text_clear_f32(td, self._tgrads, n0, ids0.data_ptr(), _lib.current_stream()),
                               "mi_pinsage_text_clear_f32")
                gb.index_fill_(0, seeds, 0.0)
        if not self.keep_grads:
            self._adam_step += 1
            steps = [self.optimizer.state[q]["step"] for q in group["params"]]
            if steps and steps[0].is_cuda:
                t._foreach_add_(steps, 1)
            else:
                for s in steps:
                    s += 1
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
    params = ([] if model.featured else [model.proj.weight]) + [x for cv in model.convs for x in (cv.Q.weight, cv.Q.bias, cv.W.weight, cv.W.bias)]
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
    for l, cv in enumerate(model.convs):
        c = d.conv[l]
        c.q_w, c.q_b, c.w_w, c.w_b = (x.data_ptr() for x in (cv.Q.weight, cv.Q.bias, cv.W.weight, cv.W.bias))
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
