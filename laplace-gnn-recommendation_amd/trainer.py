"""Fused LightGCN training step: one pass of run_pipeline_lightgcn.py:117-159 with every stage on
the GPU and no host round trip.

    forward   K fused SpMM launches (layer sum in the epilogue)      model/lightgcn.py:46-80
    sample    B edges + structured negatives on device               data/lightgcn_loader.py:95-112
    loss      gathers + BPR forward/backward in one kernel           run_pipeline_lightgcn.py:133-155
              (objective="bpr" / "softmax" and n_neg = M <= 16 negatives per positive: opt-in, SURVEY F9;
               negatives="popularity": negatives drawn ∝ degree ** neg_power, and with the softmax the logQ correction;
               negatives="in_batch": no negative is drawn, the other positives of a slot's group of in_batch_group slots
               are its negatives, scored on the f32 matrix cores — mi_inbatch_softmax_fwd_bwd_f32;
               full_softmax=True: the exact softmax over every item of the catalogue, the objective the sampled ones
               estimate — mi_full_softmax_fwd_bwd_f32; its gradient is dense over the item rows, so sparse_batch=False)
              (cl_weight > 0, sparse_batch=False: the noise-view contrastive term of XSimGCL on top of any of these — every
               layer of the step's forward perturbed by mi_perturb_rows_f32, the batch's users and positives contrasted,
               final read-out against layer cl_layer, by mi_contrastive_fwd_bwd_f32; _step_contrastive)
    backward  K SpMM launches on A^T, G/(K+1) folded in as addend    (autograd of the forward)
    update    dense Adam over the whole table, L2 term folded in     run_pipeline_lightgcn.py:157-159

Same arithmetic as the autograd path (LightGCN.forward + bpr_loss + backward + Adam); what is
removed is memory traffic: no cat, no [N,K+1,D] stack, no saved activations (the propagate is
linear), no materialised per-batch gathers, gradient and L2 term consumed in the Adam pass.

HBM-resident state (fp32, N = U+I rows of D): table, final, two ping-pong buffers, Gc, m, v.

`sparse_batch=True` (default) additionally uses what is known about the operands of one step — the
loss reads `final` only at the <= 3B batch rows, and its gradient is non-zero only there — to move
fewer bytes for the SAME result (to rounding: the layer sum is associated differently; each form is bitwise
reproducible run to run — no float atomics anywhere in the step):
  * the batch is drawn first (it does not depend on the embeddings); its unique node set and the
    node -> slot map are built on device (mi_batch_nodes_i32), no host read-back;
  * forward: layers 1..K-1 are plain products; the running layer sum is kept only at the batch rows
    (mi_gather_rows_f32); layer K is computed only at the batch rows (row_list) — hub rows still go
    through the split path;
  * the BPR kernel reads / writes compact [<= 3B, D] tables through the node map, so the dense Gc
    buffer, its zero-fill and its K reads as an addend disappear;
  * backward layer 1 gathers only the non-zero rows of its input (x_map); all layers take the compact
    gradient as addend (addend_map);
  * the last backward product IS the parameter gradient: with fuse_adam (default) the Adam update runs in
    that product's epilogue (mi_adam_args), so the gradient is never written or read back (-1.1 GB at C2).
`sparse_batch=False` is the straightforward form (full `final`, dense Gc) kept for A/B and for callers
that want the full forward output of the step.

`reorder` (default: on for adjacencies of >= 1M entries) trains under a LOCALITY ORDER of the nodes
(interactions.LocalityOrder: items by popularity, users by their coldest item): the adjacency, the interaction
CSR and — in place — the model's table are relabelled once at construction, every kernel then runs on the new ids,
and `to_original_order()` / `to_training_order()` put the table's rows back / forth (one gather of the table each;
`finish()` = to_original_order).  Batches passed to `step()` and returned by `sample()` are in ORIGINAL ids.  The
result is the same training run up to the summation order inside a row (entries are summed in column order, and
columns are renamed): equal to rounding, and still bitwise reproducible run to run.

_LightGCNTrainerBase, below, holds what this trainer shares with the user-sharded one (dist.ShardedLightGCNTrainer): the
hyper-parameters and their checks, the locality order's bookkeeping, the per-batch and optimizer state, sample() and the Adam
keywords.  The steps themselves differ in their launches and stay with each class.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch as t
from torch import Tensor

from . import ops
from .interactions import Interactions
from .model.lightgcn import LightGCN, check_layer_dtype, propagate_mean, propagate_mean_backward
from .sparse import SparseTensor


def _lib_bytes_batch_nodes(n_nodes: int) -> int:
    from . import _lib
    return int(_lib.lib().mi_batch_nodes_workspace_bytes(n_nodes))


NEGATIVES = ("uniform", "popularity", "in_batch")


class _LightGCNTrainerBase:
    """What LightGCNTrainer and dist.ShardedLightGCNTrainer share, once: the objective and hyper-parameter checks and
    assignments, the locality order's bookkeeping, the per-batch and optimizer state, sample() and the Adam keywords.
    `self.ops` is the kernel provider (this package's HIP `ops`; the sharded trainer's CPU tests inject another).  A subclass
    sets up its adjacency, `_r`, `_row_of_edge`, `neg_range` and `_sample_kw`, and writes its own steps."""
    in_batch = False   # no negative is drawn: (users, pos) batches (in-batch negatives, or the whole catalogue)
    full_softmax = False   # every item is a candidate (LightGCNTrainer, full_softmax=True); implies in_batch

    def __init__(self, model: LightGCN, kernels, *, lr: float, Lambda: float, batch_size: int, betas: Tuple[float, float],
                 eps: float, seed: int, sparse_batch: bool, objective: str, n_neg: int):
        ops.rank_objective_code(objective)   # ValueError for an unknown name
        ops.check_n_neg(n_neg)
        self.objective, self.n_neg = objective, n_neg
        self.ops = kernels
        self.model = model
        self.table = model.table()
        self.K = model.num_iterations
        self.lr, self.Lambda, self.batch_size = float(lr), float(Lambda), int(batch_size)
        self.betas, self.eps, self.seed = betas, float(eps), int(seed)
        self.sparse_batch = bool(sparse_batch)
        self.order, self.in_training_order = None, True
        self.step_count = 0

    def _alloc_state(self) -> None:
        """`final`, the two ping-pong buffers of the propagates, the per-batch tables (sparse_batch: compact [(2 + n_neg) B, D]
        ones and the node map instead of the dense gradient buffer) and the optimizer state."""
        n, d = self.table.shape
        dev = self.table.device
        self.final = t.empty(n, d, device=dev)
        self.bufs = (t.empty(n, d, device=dev), t.empty(n, d, device=dev))
        if self.sparse_batch:
            nb = (2 + self.n_neg) * self.batch_size
            self.gc = None
            self.gmap = t.empty(n, dtype=t.int32, device=dev)
            self.nodes = t.zeros(nb, dtype=t.int32, device=dev)
            self.n_nodes = t.zeros(2, dtype=t.int32, device=dev)
            self.sum_c = t.empty(nb, d, device=dev)
            self.gc_c = t.zeros(nb, d, device=dev)
        else:
            self.gc = t.zeros(n, d, device=dev)
        self.reg_w = t.zeros(n, device=dev)
        self.m = t.zeros(n, d, device=dev)
        self.v = t.zeros(n, d, device=dev)
        self.loss = t.zeros(1, device=dev)
        self.batch_idx = (t.empty(self.batch_size, dtype=t.int64, device=dev),
                          t.empty(self.batch_size, dtype=t.int64, device=dev),
                          t.empty(self.batch_size if self.n_neg == 1 else (self.batch_size, self.n_neg), dtype=t.int64, device=dev))

    # -- locality order --------------------------------------------------------------------------
    def _reorder(self, train: Interactions, item_degree: Optional[Tensor] = None) -> Interactions:
        """Take up train's locality order: the table's rows go into it, and `train` comes back relabelled."""
        self.order = train.locality_order(item_degree=item_degree)
        self._new_of_old = self.order.node_new_of_old()
        self._old_of_new = self.order.node_old_of_new()
        self.in_training_order = False
        self.to_training_order()
        return train.permuted(self.order)

    def to_training_order(self) -> None:
        """Rows of the model's table into the order the kernels train in (no-op without reorder)."""
        if self.order is not None and not self.in_training_order:
            self.table.copy_(self.table[self._old_of_new])  # new row r = old row old_of_new[r]
            self.in_training_order = True

    def to_original_order(self) -> None:
        """Rows of the model's table back under their original ids (evaluation, top-K, saving)."""
        if self.order is not None and self.in_training_order:
            self.table.copy_(self.table[self._new_of_old])
            self.in_training_order = False

    finish = to_original_order

    def _ids_to_training(self, batch):
        if batch is None:
            return batch
        if self.in_batch:   # (users, pos); a third entry is ignored, and pos stands in for it (the node set's third column)
            users, pos = batch[0], batch[1]
            if self.order is not None:
                users, pos = self.order.user_new_of_old[users], self.order.item_new_of_old[pos]
            return users, pos, pos
        users, pos, neg = batch
        if self.n_neg > 1 and (neg.dim() != 2 or neg.shape[1] != self.n_neg):
            raise ValueError(f"batch: neg [B, {self.n_neg}] expected, got {list(neg.shape)}")
        if self.order is None:
            return batch
        return self.order.user_new_of_old[users], self.order.item_new_of_old[pos], self.order.item_new_of_old[neg]

    # -- the batch and the optimizer's keywords ----------------------------------------------------
    def _sample(self) -> Tuple[Tensor, Tensor, Tensor]:
        return self.ops.sample_bpr_batch(self._r, self._row_of_edge, self.batch_size, self.neg_range, self.seed,
                                         self.step_count, out=self.batch_idx, **self._sample_kw)

    def sample(self) -> Tuple[Tensor, Tensor, Tensor]:
        """(users, pos, neg) of the next step's batch, ORIGINAL ids (the sharded trainer's: local ones)."""
        users, pos, neg = self._sample()
        if self.order is None:
            return users, pos, neg
        return self.order.user_old_of_new[users], self.order.item_old_of_new[pos], self.order.item_old_of_new[neg]

    def _adam_kw(self, step: int) -> dict:
        return dict(step=step, lr=self.lr, beta1=self.betas[0], beta2=self.betas[1], eps=self.eps)

    def decay_lr(self, gamma: float = 0.95) -> None:
        """ExponentialLR(gamma).step() (run_pipeline_lightgcn.py:104,178-179)."""
        self.lr *= gamma


class LightGCNTrainer(_LightGCNTrainerBase):
    def __init__(self, model: LightGCN, adj: SparseTensor, train: Interactions, *, lr: float, Lambda: float,
                 batch_size: int, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8, seed: int = 0,
                 neg_range: Optional[int] = None, reference_sampler_quirks: bool = False,
                 sparse_batch: bool = True, fuse_adam: bool = True, reorder: Optional[bool] = None,
                 objective: str = "reference", n_neg: int = 1, negatives: str = "uniform", neg_power: float = 0.75,
                 logq_correction: Optional[bool] = None, in_batch_group: int = 1024, full_softmax: bool = False,
                 cl_weight: float = 0.0, cl_eps: float = 0.2, cl_tau: float = 0.15, cl_layer: int = 1, cl_group: int = 1024,
                 layer_dtype: str = "f32"):
        """negatives="popularity": negatives drawn ∝ (training degree) ** neg_power from `neg_table`, built in the id space
        the kernels train in.  logq_correction: the softmax's logits become s - log q(item); None = on iff
        objective == "softmax" and negatives != "uniform".  The defaults launch the step as it was.
        negatives="in_batch" (objective="softmax", n_neg = 1: nothing is drawn): the candidates of a slot are the positives of
        its group of in_batch_group consecutive slots (a multiple of 32 in 32..4096), minus those that name the slot's own item
        or belong to its user; the user's other items in the group are NOT rejected.  The batch is the uniform sampler's edge
        stream — users and pos at a (seed, step) are the bits a negatives="uniform" trainer draws; the negative it draws as
        well is ignored.  The logQ correction's proposal is "the item of a uniformly drawn training edge", q ∝ training degree
        (ops.negative_table(degree, 1.0)); neg_power is not used.  step(batch) takes (users, pos); a third entry is ignored.
        full_softmax=True (objective="softmax", negatives="uniform", n_neg = 1, sparse_batch=False passed explicitly, no
        logq_correction, no reference_sampler_quirks, neg_range None or num_items): the exact softmax over all num_items items,
        nothing drawn and nothing corrected.  Batches are the uniform sampler's users and pos at the same (seed, step), as for
        negatives="in_batch"; the step is the dense one, whose gradient buffer the loss fills at every item row.
        cl_weight > 0 (sparse_batch=False passed explicitly, K >= 1): the noise-view contrastive term of XSimGCL is added to
        whatever main loss the other keywords choose — loss + cl_weight * (L_user + L_item).  Every propagated layer of the
        step's forward is perturbed by cl_eps * sign(x) * (unit noise keyed on (seed, step, layer, ORIGINAL node id)), and the
        batch's user nodes and positive item nodes are each contrasted, final read-out against layer cl_layer (1..K), at
        temperature cl_tau in groups of cl_group consecutive slots (a multiple of 32 in 32..4096).  The rule is in
        include/laplace_hip.h, "Noise-view contrastive term".  forward(), evaluation and serving stay unperturbed; cl_weight = 0
        (the default) launches the step as it was.
        layer_dtype="bf16" (opt-in mixed precision; d % 8 == 0, d <= 256, cl_weight = 0): the layers of the step's forward are
        kept in bf16 under the rule of include/laplace_hip.h, "bf16 layer tables" — X_0 = rn(table), X_k = rn(A X_{k-1}) for
        k < K, read-out c * (E0 + X_1 + ... + X_{K-1} + A X_{K-1}) in f32.  The master table, the loss, the backward products
        (those of the unrounded linear map: the rounding is treated as the identity) and Adam stay f32.  Both step forms, every
        objective, n_neg, negatives, full_softmax and reorder.  forward() keeps returning the f32 forward, so evaluation and
        serving do not change; forward(layer_dtype="bf16") returns what the step trains on.  "f32" (the default) launches the
        step as it was."""
        super().__init__(model, ops, lr=lr, Lambda=Lambda, batch_size=batch_size, betas=betas, eps=eps, seed=seed,
                         sparse_batch=sparse_batch, objective=objective, n_neg=n_neg)
        if negatives not in NEGATIVES:
            raise ValueError(f"negatives must be one of {NEGATIVES}, got {negatives!r}")
        if isinstance(neg_power, bool) or not isinstance(neg_power, (int, float)) or not 0.0 <= neg_power <= 1.0:
            raise ValueError(f"neg_power must be a number in [0, 1], got {neg_power!r}")
        if logq_correction is None:
            logq_correction = objective == "softmax" and negatives in ("popularity", "in_batch")
        elif logq_correction and objective != "softmax":
            raise ValueError(f"logq_correction corrects the sampled softmax, not objective={objective!r}")
        if negatives == "popularity":
            if reference_sampler_quirks:
                raise ValueError('negatives="popularity" does not combine with reference_sampler_quirks')
            if neg_range is not None and int(neg_range) != model.num_items:
                raise ValueError(f'negatives="popularity" draws from every item: neg_range {neg_range} != {model.num_items}')
        if negatives == "in_batch":
            ops.check_inbatch_group(in_batch_group)
            if objective != "softmax":
                raise ValueError(f'negatives="in_batch" is a sampled softmax: objective="softmax" expected, got {objective!r}')
            if n_neg != 1:
                raise ValueError(f'negatives="in_batch" draws nothing: n_neg stays 1, got {n_neg}')
            if reference_sampler_quirks:
                raise ValueError('negatives="in_batch" does not combine with reference_sampler_quirks')
            if neg_range is not None and int(neg_range) != model.num_items:
                raise ValueError(f'negatives="in_batch" takes its negatives from the batch: neg_range {neg_range} != {model.num_items}')
        if full_softmax:
            if objective != "softmax":
                raise ValueError(f'full_softmax is the exact softmax: objective="softmax" expected, got {objective!r}')
            if negatives != "uniform":
                raise ValueError(f'full_softmax draws nothing: negatives stays "uniform", got {negatives!r}')
            if n_neg != 1:
                raise ValueError(f"full_softmax draws nothing: n_neg stays 1, got {n_neg}")
            if reference_sampler_quirks:
                raise ValueError("full_softmax does not combine with reference_sampler_quirks")
            if neg_range is not None and int(neg_range) != model.num_items:
                raise ValueError(f"full_softmax scores every item: neg_range {neg_range} != {model.num_items}")
            if logq_correction:
                raise ValueError("full_softmax samples nothing: logq_correction has nothing to correct")
            if sparse_batch:
                raise ValueError("full_softmax has a gradient at every item row: pass sparse_batch=False")
            self.full_softmax = True
        self.in_batch = negatives == "in_batch" or self.full_softmax
        if isinstance(cl_weight, bool) or not isinstance(cl_weight, (int, float)) or not 0.0 <= cl_weight < math.inf:
            raise ValueError(f"cl_weight must be a finite number >= 0, got {cl_weight!r}")
        self.cl_weight = float(cl_weight)
        if self.cl_weight > 0.0:
            ops.check_contrastive(model.embedding_dim, eps=cl_eps, tau=cl_tau, group=cl_group)
            if self.K == 0:
                raise ValueError("cl_weight > 0 contrasts a propagated layer: num_iterations >= 1 expected, got K = 0")
            if isinstance(cl_layer, bool) or not isinstance(cl_layer, int) or not 1 <= cl_layer <= self.K:
                raise ValueError(f"cl_layer must be an integer in 1..{self.K}, got {cl_layer!r}")
            if sparse_batch:
                raise ValueError("cl_weight > 0 perturbs whole layers, the dense step: pass sparse_batch=False")
            self.cl_eps, self.cl_tau, self.cl_layer, self.cl_group = float(cl_eps), float(cl_tau), cl_layer, cl_group
        check_layer_dtype(layer_dtype, model.embedding_dim)
        if layer_dtype == "bf16" and self.cl_weight > 0.0:
            raise ValueError('layer_dtype="bf16" does not combine with cl_weight > 0: the perturbation kernel is f32')
        self.layer_dtype = layer_dtype
        self.in_batch_group = int(in_batch_group) if negatives == "in_batch" else None
        self.negatives, self.neg_power, self.logq_correction = negatives, float(neg_power), bool(logq_correction)
        if not self.table.is_cuda:
            raise RuntimeError("LightGCNTrainer needs the model on the GPU (model.to('cuda')); no CPU fallback")
        # reference: num_nodes = max(train item id)  => negatives in [0, max_item_id)  (Appendix A.3)
        self.neg_range = int(neg_range) if neg_range is not None else train.num_items
        self.quirk = bool(reference_sampler_quirks)
        # a negative range that is not "every item" names items by id: it does not survive a relabelling
        can_reorder = self.neg_range == train.num_items and not self.quirk
        if reorder is None:
            reorder = can_reorder and adj.nnz() >= ops.PLAN_MIN_NNZ
        elif reorder and not can_reorder:
            raise ValueError("reorder=True needs neg_range == num_items and no reference sampler quirks")
        if reorder:
            train = self._reorder(train)
            adj = adj.permuted(self._new_of_old)
        self.adj_fwd, self.adj_bwd = adj.gcn_normalized(model.add_self_loops)
        if self.order is not None:
            # items are numbered by popularity: their first rows take half of all user-row gathers — dense launches keep
            # them in LDS (ops.spmm, `hot`; a speed hint, results unchanged)
            self.adj_fwd.hot = self.adj_bwd.hot = ops.hot_item_rows(model.num_users, model.num_items)
        self.train = train
        self.fuse_adam = bool(fuse_adam)
        self._alloc_state()
        self.buf_a, self.buf_b = self.bufs
        dev = self.table.device
        if self.sparse_batch:
            self.final_c = t.empty(self.sum_c.shape, device=dev)
            self._nodes_ws = t.empty(_lib_bytes_batch_nodes(self.table.shape[0]), dtype=t.uint8, device=dev)
        self._r = train.csr()
        self._row_of_edge = train.row_of_edge()
        # the proposal of the negatives and its log, by TRAINING id (`train` is already relabelled here)
        self.neg_table, self.logq = None, None
        if self.negatives == "popularity":
            degree = t.bincount(self._r.col.long(), minlength=train.num_items)
            self.neg_table = ops.negative_table(degree, self.neg_power, device=dev)
        if self.logq_correction and self.in_batch:   # the item of a uniformly drawn training edge: q ∝ degree
            degree = t.bincount(self._r.col.long(), minlength=train.num_items)
            self.logq = ops.negative_table(degree, 1.0, device=dev).logq
        elif self.logq_correction:   # uniform negatives: q = 1 / neg_range for every item
            self.logq = (self.neg_table.logq if self.neg_table is not None
                         else t.full((train.num_items,), -math.log(self.neg_range), dtype=t.float32, device=dev))
        self._sample_kw = (dict(n_neg=self.n_neg, table=self.neg_table) if self.neg_table is not None
                           else dict(quirk=self.quirk, n_neg=self.n_neg))
        if self.cl_weight > 0.0:
            # layer cl_layer of the perturbed forward (the backward's h_K when cl_layer == K); dL_cl/dX_{cl_layer}, all zero
            # between steps: a step writes the batch's rows and zeroes them again; the two sides' losses
            self.x_cl = t.empty_like(self.final)
            self.g_cl = t.zeros_like(self.final)
            self.cl_loss = t.zeros(2, device=dev)
        # bf16 layer tables beside the f32 buffers the backward keeps: X_0 and a ping-pong pair; K <= 1 stores no layer
        self.x_bf16 = ()
        if self.layer_dtype == "bf16":
            n_tab = 0 if self.K == 0 else min(self.K, 3)
            self.x_bf16 = tuple(t.empty(self.table.shape, dtype=t.bfloat16, device=dev) for _ in range(n_tab))

    # -- pieces (also used one by one in tests) ------------------------------------------------
    def forward(self, layer_dtype: str = "f32") -> Tensor:
        """mean_k(A^k E0) over the whole table; rows in TRAINING order (index with order.node_new_of_old()).  The f32 forward
        whatever the trainer's layer_dtype (evaluation, serving); layer_dtype="bf16" = the forward a bf16 step trains on."""
        self.to_training_order()
        if layer_dtype != "f32":
            check_layer_dtype(layer_dtype, self.table.shape[1])
            return propagate_mean(self.adj_fwd, self.table, self.K, out=self.final, scratch=self.x_bf16 or None,
                                  layer_dtype=layer_dtype)
        return propagate_mean(self.adj_fwd, self.table, self.K, out=self.final, scratch=(self.buf_a, self.buf_b))

    def _loss(self, users, pos, neg, final, **kw) -> None:
        """Loss and its gradient on `final` (self.logq is None without the logQ correction)."""
        if self.in_batch:
            if self.full_softmax:
                ops.full_softmax_fwd_bwd(users, pos, final, self.table, self.model.num_users, self.Lambda, reg_w=self.reg_w,
                                         loss_out=self.loss, **kw)
                return
            ops.inbatch_softmax_fwd_bwd(users, pos, final, self.table, self.model.num_users, self.Lambda,
                                        group=self.in_batch_group, reg_w=self.reg_w, loss_out=self.loss, logq=self.logq, **kw)
            return
        ops.rank_loss_fwd_bwd(users, pos, neg, final, self.table, self.model.num_users, self.Lambda,
                              objective=self.objective, reg_w=self.reg_w, loss_out=self.loss, logq=self.logq, **kw)

    def _batch(self) -> Tuple[Tensor, Tensor, Tensor]:
        """The step's own batch: _sample(), with pos in place of the drawn negatives when they come from the batch."""
        users, pos, neg = self._sample()
        return (users, pos, pos) if self.in_batch else (users, pos, neg)

    def step(self, batch: Optional[Tuple[Tensor, Tensor, Tensor]] = None) -> Tensor:
        """One training iteration; returns the loss as a 1-element device tensor (no sync).  batch: original ids."""
        self.to_training_order()
        batch = self._ids_to_training(batch)
        if self.sparse_batch:
            return self._step_sparse(batch)
        if self.cl_weight > 0.0:
            return self._step_contrastive(batch)
        K = self.K
        self.forward(self.layer_dtype)
        users, pos, neg = batch if batch is not None else self._batch()
        self.gc.zero_()
        self.reg_w.zero_()
        self._loss(users, pos, neg, self.final, g_final=self.gc, g_scale=1.0 / (K + 1))
        g0 = propagate_mean_backward(self.adj_bwd, self.gc, K, scratch=(self.buf_a, self.buf_b), pre_scaled=True)
        self.step_count += 1
        ops.adam_step(self.table, g0, self.m, self.v, reg_w=self.reg_w, **self._adam_kw(self.step_count))
        return self.loss

    def _step_contrastive(self, batch: Optional[Tuple[Tensor, Tensor, Tensor]]) -> Tensor:
        """The dense step with the noise-view contrastive term: K products each followed by ops.perturb_rows (which also
        folds the layer into `final`), the main loss as it is, the two contrast calls adding to its gradient buffer, and the
        backward h_k = gc + A^T h_{k+1} with cl_weight * dL_cl/dX_l added at layer l = cl_layer."""
        K, l, tab, c, w = self.K, self.cl_layer, self.table, 1.0 / (self.K + 1), self.cl_weight
        users, pos, neg = batch if batch is not None else self._batch()
        row_ids = self._old_of_new if self.order is not None else None
        x = tab
        for k in range(1, K + 1):
            y = self.x_cl if k == l else self.bufs[k % 2]
            ops.spmm(self.adj_fwd, x, Y=y)
            ops.perturb_rows(y, eps=self.cl_eps, layer=k, seed=self.seed, step=self.step_count, row_ids=row_ids,
                             addend=tab if k == 1 else self.final, S=self.final, scale=c if k == K else 1.0)
            x = y
        self.gc.zero_()
        self.reg_w.zero_()
        self._loss(users, pos, neg, self.final, g_final=self.gc, g_scale=c)
        nodes = t.cat([users, pos + self.model.num_users])
        B = users.numel()
        for side in range(2):
            ops.contrastive_fwd_bwd(nodes[side * B:(side + 1) * B], self.final, self.x_cl, tau=self.cl_tau, group=self.cl_group,
                                    g_a=self.gc, g_b=self.g_cl, g_scale_a=w * c, g_scale_b=w, loss_out=self.cl_loss[side:side + 1])
        self.loss.add_(self.cl_loss.sum(), alpha=w)

        def add_layer_gradient(h):   # h[node] += g_cl[node] at the batch's nodes; a node named twice writes one value twice
            h[nodes] = h[nodes] + self.g_cl[nodes]
            self.g_cl[nodes] = 0.0
        cur = self.gc
        if l == K:                   # x_cl is free again: it holds h_K = gc + G
            cur = self.x_cl.copy_(self.gc)
            add_layer_gradient(cur)
        for k in range(K - 1, -1, -1):
            nxt = self.bufs[k % 2]
            ops.spmm(self.adj_bwd, cur, addend=self.gc, S=nxt)
            if k == l:
                add_layer_gradient(nxt)
            cur = nxt
        self.step_count += 1
        ops.adam_step(tab, cur, self.m, self.v, reg_w=self.reg_w, **self._adam_kw(self.step_count))
        return self.loss

    def _step_sparse(self, batch: Optional[Tuple[Tensor, Tensor, Tensor]]) -> Tensor:
        K, tab, adj, adj_t = self.K, self.table, self.adj_fwd, self.adj_bwd
        users, pos, neg = batch if batch is not None else self._batch()
        if users.numel() != self.batch_size:
            raise ValueError("batch size differs from the trainer's")
        gmap, nodes, cnt2 = ops.batch_nodes(users, pos, neg, self.model.num_users, tab.shape[0], gmap=self.gmap,
                                            nodes=self.nodes, count=self.n_nodes, ws=self._nodes_ws)
        cnt = cnt2[:1]
        # ---- forward: final only at the batch rows
        c = 1.0 / (K + 1)
        ops.gather_rows(self.sum_c, tab, nodes, cnt)                      # S_c = E0[batch rows]
        x = tab
        bufs = (self.buf_a, self.buf_b)
        bf16 = self.layer_dtype == "bf16" and K >= 1
        spmm = ops.spmm_bf16 if bf16 else ops.spmm
        if bf16:                                                          # X_0 = rn(E0); the layers ping-pong in bf16
            x = ops.rows_to_bf16(tab, out=self.x_bf16[0])
        for k in range(1, K):                                             # layers 1..K-1: plain products
            y = self.x_bf16[1 + (k - 1) % 2] if bf16 else bufs[(k - 1) % 2]
            spmm(adj, x, Y=y)
            ops.gather_rows(self.sum_c, y, nodes, cnt, accumulate=True)   # S_c += X_k[batch rows]
            x = y
        if K >= 1:                                                        # layer K at the batch rows only
            spmm(adj, x, addend=self.sum_c, S=self.final_c, scale=c, row_list=nodes, n_list_dev=cnt)
            final_c = self.final_c
        else:
            final_c = self.sum_c
        # ---- loss + its gradient on the compact tables
        self.gc_c.zero_()
        self.reg_w.zero_()
        self._loss(users, pos, neg, final_c, g_final=self.gc_c, g_scale=c, node_map=gmap)
        # ---- backward: g_K = Gc (compact); g_k = Gc + A^T g_{k+1}
        if K == 0:
            g0 = self.buf_a
            g0.zero_()
            g0.index_add_(0, nodes[: int(cnt)].long(), self.gc_c[: int(cnt)])  # K = 0 is not a hot path
        else:
            cur = None
            for i in range(K):
                nxt = bufs[i % 2]
                # the last product's output is the parameter gradient: Adam consumes it in the epilogue
                opt = None
                if i == K - 1 and self.fuse_adam:
                    opt = dict(p=tab, m=self.m, v=self.v, reg_w=self.reg_w, **self._adam_kw(self.step_count + 1))
                out = None if opt is not None else nxt
                if i == 0:   # input = the compact gradient itself: skip its all-zero rows
                    # (the split rows are the hub ITEMS': their columns are users, of which the batch names few)
                    ops.spmm(adj_t, self.gc_c, addend=self.gc_c, S=out, x_map=gmap, addend_map=gmap, adam=opt,
                             x_rare=8 * self.batch_size <= self.model.num_users)
                else:
                    ops.spmm(adj_t, cur, addend=self.gc_c, S=out, addend_map=gmap, adam=opt)
                cur = nxt
            g0 = cur
        self.step_count += 1
        if K == 0 or not self.fuse_adam:
            ops.adam_step(tab, g0, self.m, self.v, reg_w=self.reg_w, **self._adam_kw(self.step_count))
        return self.loss
