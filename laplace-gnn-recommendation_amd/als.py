"""Implicit-feedback matrix factorisation by alternating least squares (iALS: Hu, Koren and Volinsky, ICDM 2008; Rendle et
al., RecSys 2022) — the trained baseline a LightGCN figure is read against, and a candidate source that sees a new
interaction without a build step (fold_in).

The model is two embedding tables with LightGCN's attribute surface (users_emb / items_emb / num_users / num_items), so
topk_for_users, ops.rank_of_items, get_full_rank_metrics_lightgcn, save_predictions and data.matching.LightGCNMatcher take it
unchanged.  A half-sweep is ONE launch of ops.als_solve_rows (csrc/als.hip; the rule is stated in include/laplace_hip.h) after
one d x d Gram product (ops.gemm): with the other table Y fixed, row r becomes the solution of
    (Y^T Y + alpha * sum_e y_e y_e^T + reg I) x = (1 + alpha) * sum_e y_e        over the entries e of row r.
With solver="block" the one launch is ops.als_block_rows (csrc/als_block.hip, "iALS block" in the header) instead: a row-local
iALS++ (Rendle et al., RecSys 2021) that warm-starts from the table and minimises the same row quadratic exactly over one
block of `block` coordinates at a time, `block_sweeps` passes per half-sweep; it is the only solver for dim > 128 (up to 256).
One wavefront walks a row there, so a popular item's row is a half-sweep of its own: hub_threshold=T (opt-in, block solver
only) takes every row with more than T entries from its dim x dim system instead, assembled once over one workgroup per chunk
of the row ("iALS block hub" in the header); the other rows, and hub_threshold=None, keep every bit.

Per-edge confidences (Hu, Koren and Volinsky: c_ui = 1 + alpha r_ui) and frequency-scaled regularisation (Rendle et al.,
RecSys 2022, section 4) are opt-in: bind / fit / fold_in take a `confidence` per edge and the model a `reg_power`; with either
in use the one launch is the weighted entry of the same solver ("iALS weighted" / "iALS block weighted" in the header), which
solves (Y^T Y + sum_e a_e y_e y_e^T + reg_r I) x = sum_e (1 + a_e) y_e with a_e = alpha * confidence_e.  With neither, every call
and every bit is the unweighted entry's.

Not built: the CG solver, the paper's block-outer schedule of iALS++ (all rows inside one block step, predictions of all
pairs kept between steps), a second stream for the hub rows, an automatic hub_threshold, dim > 256, a sharded form, bf16,
negative or missing-preference (p = 0) observed entries, and the matcher's entry in get_matchers / tools/e2e_hm_scale.py's
chain.
"""
from __future__ import annotations

from typing import Callable, Optional, Tuple

import torch as t
from torch import Tensor

from . import ops
from .interactions import Interactions
from .reporting.types import Stats

SIDES = ("users", "items")
SOLVERS = ("cholesky", "block")


def check_reg_power(reg_power) -> float:
    try:
        v = float(reg_power)
        ok = 0.0 <= v <= 1.0   # False for NaN
    except (TypeError, ValueError):
        v, ok = reg_power, False
    if not ok or isinstance(reg_power, bool):
        raise ValueError(f"reg_power must be a number in [0, 1], got {reg_power!r}")
    return v


def edge_confidence(confidence, n_edges: int, alpha: float, device=None) -> Tensor:
    """a_e = alpha * w_e for a per-edge weight w_e >= 0, formed in float64 and rounded to float32 once.  ValueError for
    anything but a floating tensor [n_edges] of finite, non-negative numbers (one read-back)."""
    if not isinstance(confidence, Tensor) or not confidence.is_floating_point():
        raise ValueError(f"confidence must be a floating-point tensor [{n_edges}], got "
                         f"{getattr(confidence, 'dtype', type(confidence))}")
    if confidence.dim() != 1 or confidence.numel() != n_edges:
        raise ValueError(f"confidence must have one weight per edge, shape [{n_edges}], got {tuple(confidence.shape)}")
    w = confidence.detach()
    if device is not None:
        w = w.to(device)
    if n_edges and bool((~t.isfinite(w) | (w < 0)).any().item()):
        raise ValueError("confidence must be finite and >= 0 on every edge")
    return (w.double() * float(alpha)).to(t.float32).contiguous()


def reg_rows_of(ptr: Tensor, conf: Tensor, n_cols: int, reg: float, reg_power: float) -> Tensor:
    """reg_r = reg * (n_cols + sum_e a_e)^reg_power for every row of a CSR (ptr [n_rows + 1], conf [nnz] by entry position):
    float64 torch on the tensors' device, rounded to float32 once.  The row sums are differences of ONE float64 running sum
    over the entries (no atomics: equal bits run to run)."""
    run = t.zeros(conf.numel() + 1, dtype=t.float64, device=conf.device)
    run[1:] = t.cumsum(conf.double(), 0)
    p = ptr.long()
    mass = float(n_cols) + (run[p[1:]] - run[p[:-1]])
    return (float(reg) * mass.pow(float(reg_power))).to(t.float32).contiguous()


class ImplicitALS(t.nn.Module):
    """iALS with confidence 1 + alpha on the observed pairs and 1 on all others, L2 weight reg on both tables.  A pair that
    occurs twice in `interactions` counts twice (the kernel sums a row's entries as written); the pipeline's graphs are
    deduplicated.

    bind / fit / fold_in take `confidence`: a weight w_e >= 0 per edge (a count, a recency weight), in edge_index order; the
    pair's confidence is then 1 + a_e with a_e = alpha * w_e (float32, rounded once at bind).  confidence=None is w_e = 1.

    reg_power = nu in [0, 1] scales a row's regulariser by its TOTAL confidence over the fixed table:
        reg_r = reg * (n_cols + sum_e a_e)^nu,        n_cols the number of rows of the other table.
    That is the frequency-scaled term lambda (|I_u| + alpha0 |I|)^nu of Rendle et al. (RecSys 2022, section 4) in this
    project's scaling, where an unobserved pair weighs 1 and an observed one 1 + a_e: the paper's weights are alpha0 and 1, so
    the two agree up to the constant alpha0^nu with alpha0 = 1 / alpha.  The factor is between n_cols^nu and (n_cols + mass)^nu,
    i.e. in the thousands at nu = 1: `reg` MUST be rescaled (retuned) with nu; a reg tuned at nu = 0 is far too strong at
    nu > 0.  nu = 0 (the default) is the one reg of every row.

    hub_threshold (solver="block" only; None = off): every half_sweep, fit and fold_in takes the rows with more entries than
    this from their assembled system (ops.als_block_rows(hub_threshold=)).  profiles/als_hub.md has what it buys."""

    def __init__(self, num_users: int, num_items: int, dim: int = 64, alpha: float = 1.0, reg: float = 20.0, seed: int = 0,
                 init_std: float = 0.1, solver: str = "cholesky", block: int = 16, block_sweeps: int = 1,
                 fold_in_sweeps: int = 4, reg_power: float = 0.0, hub_threshold: Optional[int] = None):
        super().__init__()
        self.reg_power = check_reg_power(reg_power)
        if solver not in SOLVERS:
            raise ValueError(f"solver must be one of {SOLVERS}, got {solver!r}")
        ops.check_als_hub_threshold(hub_threshold, solver)
        self.hub_threshold = None if hub_threshold is None else int(hub_threshold)
        if solver == "block":
            ops.check_als_block(dim, block, block_sweeps, alpha, reg)
            ops.check_als_block(dim, block, fold_in_sweeps, alpha, reg)
        else:
            if isinstance(dim, int) and dim > ops.ALS_MAX_DIM:
                raise ValueError(f"dim {dim} > {ops.ALS_MAX_DIM} requires solver=\"block\" (the Cholesky solver holds one "
                                 f"dim x dim system per workgroup in LDS)")
            ops.check_als(dim, alpha, reg)
        self.solver, self.block = solver, int(block)
        self.block_sweeps, self.fold_in_sweeps = int(block_sweeps), int(fold_in_sweeps)
        self.num_users, self.num_items, self.dim = int(num_users), int(num_items), int(dim)
        self.alpha, self.reg = float(alpha), float(reg)
        gen = t.Generator().manual_seed(int(seed))   # drawn on the host: the same tables whatever the device
        self.users_emb = t.nn.Embedding(self.num_users, self.dim)
        self.items_emb = t.nn.Embedding(self.num_items, self.dim)
        for emb in (self.users_emb, self.items_emb):
            emb.weight.requires_grad_(False)
            emb.weight.copy_(t.randn(emb.weight.shape, generator=gen) * float(init_std))
        self._bound: Optional[Tuple[Interactions, ops.DeviceCSR, ops.DeviceCSR]] = None
        self._bound_conf: Optional[Tensor] = None   # the `confidence` object of the bind
        # weighted binds only: the edge-order a_e, and per side (conf by entry position, reg_rows or None)
        self._weights: Optional[Tuple[Tensor, Tuple[Tensor, Optional[Tensor]], Tuple[Tensor, Optional[Tensor]]]] = None

    # ---- the graph -----------------------------------------------------------------------------------------------------
    def bind(self, interactions: Interactions, confidence: Optional[Tensor] = None) -> None:
        """The training graph of the half-sweeps that follow: its users x items CSR and, built once, the transposed one.
        `confidence` [E] (edge_index order) is validated once (one read-back) and carried into the user CSR through its perm
        and into the transposed CSR through perm_t; with reg_power != 0 the per-row regularisers of both sides are formed
        here, in float64 on the device."""
        if self._bound is not None and self._bound[0] is interactions and self._bound_conf is confidence:
            return
        if interactions.num_users != self.num_users or interactions.num_items != self.num_items:
            raise ValueError(f"interactions are {interactions.num_users} x {interactions.num_items}, the model "
                             f"{self.num_users} x {self.num_items}")
        dev = self.items_emb.weight.device
        a_edge = None if confidence is None else edge_confidence(confidence, interactions.num_edges, self.alpha, dev)
        inter = interactions.to(dev)
        if a_edge is None:
            by_user = inter.csr()
        else:   # its own CSR: the cached one has no perm
            by_user = ops.coo_to_csr(inter.edge_index[0].contiguous(), inter.edge_index[1].contiguous(), self.num_users,
                                     self.num_items, want_perm=True)
        by_item = ops.csr_transpose(by_user)
        self._weights = None
        if a_edge is not None or self.reg_power != 0.0:
            if a_edge is None:
                a_edge = t.full((by_user.nnz,), self.alpha, dtype=t.float32, device=dev)
                conf_u = a_edge
            else:
                conf_u = a_edge[by_user.perm.long()].contiguous()
            conf_i = conf_u[by_item.perm.long()].contiguous()
            reg_u = reg_i = None
            if self.reg_power != 0.0:
                reg_u = reg_rows_of(by_user.rowptr, conf_u, self.num_items, self.reg, self.reg_power)
                reg_i = reg_rows_of(by_item.rowptr, conf_i, self.num_users, self.reg, self.reg_power)
            self._weights = (a_edge, (conf_u, reg_u), (conf_i, reg_i))
        self._bound, self._bound_conf = (interactions, by_user, by_item), confidence

    def _tables(self, side: str) -> Tuple[Tensor, Tensor]:
        if side not in SIDES:
            raise ValueError(f"side must be one of {SIDES}, got {side!r}")
        mine, other = (self.users_emb, self.items_emb) if side == "users" else (self.items_emb, self.users_emb)
        return mine.weight.data, other.weight.data

    def _solve(self, csr: ops.DeviceCSR, fixed: Tensor, out: Optional[Tensor], conf: Optional[Tensor] = None,
               reg_rows: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
        """`out` is the table of a half-sweep (the block solver's start as well) or None for a fold-in (a zero start).
        conf / reg_rows None: the unweighted entry."""
        gram = ops.gemm(fixed, fixed, trans_a=True, trans_b=False)
        if self.solver == "block":
            return ops.als_block_rows(csr, fixed, gram, alpha=self.alpha, reg=self.reg, block=self.block, x=out,
                                      sweeps=self.block_sweeps if out is not None else self.fold_in_sweeps,
                                      conf=conf, reg_rows=reg_rows, hub_threshold=self.hub_threshold)
        return ops.als_solve_rows(csr, fixed, gram, alpha=self.alpha, reg=self.reg, out=out, conf=conf, reg_rows=reg_rows)

    def half_sweep(self, side: str, interactions: Optional[Interactions] = None, confidence: Optional[Tensor] = None
                   ) -> Tensor:
        """Re-solves every row of one table against the other.  Returns the device counter of rows whose factorisation
        failed (int32 [1]; those rows are zero) without reading it: fit() reads it once per epoch."""
        if interactions is not None:
            self.bind(interactions, confidence)
        if self._bound is None:
            raise RuntimeError("half_sweep needs a graph: pass interactions, or call bind() / fit() first")
        mine, other = self._tables(side)
        k = 1 if side == "users" else 2
        conf, reg_rows = self._weights[k] if self._weights is not None else (None, None)
        return self._solve(self._bound[k], other, mine, conf, reg_rows)[1]

    def fit(self, interactions: Interactions, epochs: int, callback: Optional[Callable[[int, "ImplicitALS"], None]] = None,
            confidence: Optional[Tensor] = None) -> "ImplicitALS":
        """`epochs` times a user half-sweep, then an item half-sweep.  callback(epoch, model) runs after each epoch.
        `confidence`: see bind()."""
        self.bind(interactions, confidence)
        for epoch in range(int(epochs)):
            failed = self.half_sweep("users") + self.half_sweep("items")
            n = int(failed.item())   # the epoch's one read-back
            if n:
                raise RuntimeError(f"iALS epoch {epoch}: {n} row systems met a non-positive or non-finite pivot "
                                   f"(alpha={self.alpha}, reg={self.reg}); the rows were zeroed")
            if callback is not None:
                callback(epoch, self)
        return self

    def fold_in(self, ptr: Tensor, idx: Tensor, confidence: Optional[Tensor] = None) -> Tensor:
        """Vectors [len(ptr) - 1, dim] for rows that are not in the model — an int32 CSR (ptr, idx) over ITEM ids — against
        the current item table: a user half-sweep on another CSR, so a new interaction is seen at once.  The block solver
        starts these rows from zero and makes fold_in_sweeps passes over them.  `confidence` [len(idx)] holds the weights
        w_e in idx order (None: 1); with reg_power != 0 each row's reg is scaled by that row's OWN mass,
        reg * (num_items + sum_e a_e)^reg_power over the entries given here."""
        csr = ops.DeviceCSR(int(ptr.numel()) - 1, self.num_items, ptr, idx)
        conf = reg_rows = None
        if confidence is not None or self.reg_power != 0.0:
            conf = (t.full((csr.nnz,), self.alpha, dtype=t.float32, device=idx.device) if confidence is None
                    else edge_confidence(confidence, csr.nnz, self.alpha, idx.device))
            if self.reg_power != 0.0:
                reg_rows = reg_rows_of(ptr, conf, self.num_items, self.reg, self.reg_power)
        x, failed = self._solve(csr, self.items_emb.weight.data, None, conf, reg_rows)
        n = int(failed.item())
        if n:
            raise RuntimeError(f"iALS fold-in: {n} row systems met a non-positive or non-finite pivot")
        return x

    # ---- for tests and logs ----------------------------------------------------------------------------------------------
    def objective(self, interactions: Interactions, edge_block: int = 1 << 20, confidence: Optional[Tensor] = None) -> float:
        """The iALS objective, halved so that a row's share is 1/2 x^T A x - b^T x + const with the A and b of the rule:
            1/2 * sum over ALL (u, i) of c_ui (p_ui - x_u . y_i)^2  +  1/2 * (sum_u reg_u |x_u|^2 + sum_i reg_i |y_i|^2),
        c = 1 + a_e, p = 1 on the observed pairs (every occurrence of a repeated pair), c = 1, p = 0 elsewhere; a_e = alpha and
        reg_r = reg without weights.  With `interactions` the bound graph (and confidence None or the bound one) the a_e and
        reg_r are the float32 values the half-sweeps use; otherwise they are formed from `confidence` as bind() forms them.
        float64 torch on the device, through the Gram matrix: not on the hot path."""
        X = self.users_emb.weight.data.double()
        Y = self.items_emb.weight.data.double()
        ei = interactions.edge_index.to(X.device)
        a_edge = reg_u = reg_i = None
        if (self._bound is not None and self._bound[0] is interactions and (confidence is None or confidence is self._bound_conf)):
            if self._weights is not None:
                a_edge, (_, reg_u), (_, reg_i) = self._weights
        elif confidence is not None or self.reg_power != 0.0:
            a_edge = (t.full((ei.shape[1],), self.alpha, dtype=t.float32, device=X.device) if confidence is None
                      else edge_confidence(confidence, ei.shape[1], self.alpha, X.device))
            if self.reg_power != 0.0:
                mass = [t.zeros(n, dtype=t.float64, device=X.device).index_add_(0, ei[k], a_edge.double())
                        for k, n in ((0, self.num_users), (1, self.num_items))]
                reg_u = (self.reg * (self.num_items + mass[0]).pow(self.reg_power)).to(t.float32)
                reg_i = (self.reg * (self.num_users + mass[1]).pow(self.reg_power)).to(t.float32)
        total = ((X @ (Y.T @ Y)) * X).sum()   # sum over all pairs of (x . y)^2
        for e0 in range(0, ei.shape[1], edge_block):
            u, i = ei[0, e0:e0 + edge_block], ei[1, e0:e0 + edge_block]
            s = (X[u] * Y[i]).sum(dim=1)
            c = 1.0 + (self.alpha if a_edge is None else a_edge[e0:e0 + edge_block].double())
            total = total + (c * (1.0 - s) ** 2 - s * s).sum()
        for tab, reg_r in ((X, reg_u), (Y, reg_i)):
            sq = (tab * tab).sum(dim=1)
            total = total + (self.reg * sq.sum() if reg_r is None else (reg_r.double() * sq).sum())
        return 0.5 * float(total)


def train(config, *, edge_index: Tensor, num_users: int, num_articles: int, dim: int = 64, alpha: float = 1.0,
          reg: float = 20.0, epochs: int = 3, seed: int = 0, device: str = "cuda", save_dir: Optional[str] = None,
          full_rank_ks: Optional[Tuple[int, ...]] = (12, 100), verbose: bool = True, solver: str = "cholesky",
          block: int = 16, block_sweeps: int = 1, reg_power: float = 0.0, hub_threshold: Optional[int] = None) -> Stats:
    """run_pipeline_lightgcn.train with iALS in the trainer's place: the same split (create_dataloaders_lightgcn), the ranking
    metrics @ config.k on validation and test, evaluation_full_rank on the test split and save_predictions — the same three
    files (lightgcn_output.pt and the two tables) that data.matching.LightGCNMatcher consumes.  Stats.loss is the objective
    on the training edges.  reg_power and hub_threshold go to the model.  There is no `confidence` here: the loader's split returns the three
    edge sets without the permutation that cut them, so a weight per edge of `edge_index` could not be cut alike; split
    first and call ImplicitALS.fit(interactions, epochs, confidence=) for per-edge weights."""
    from .data.lightgcn_loader import create_dataloaders_lightgcn
    from .run_pipeline_lightgcn import evaluation_full_rank, save_predictions
    from .utils.metrics_lightgcn import get_metrics_lightgcn
    (_, _, _, train_edges, val_edges, test_edges, all_edges, num_users,
     num_articles) = create_dataloaders_lightgcn(edge_index, num_users, num_articles, compat="bipartite", device=device)
    model = ImplicitALS(num_users, num_articles, dim=dim, alpha=alpha, reg=reg, seed=seed, solver=solver, block=block,
                        block_sweeps=block_sweeps, reg_power=reg_power, hub_threshold=hub_threshold).to(device)
    inter = Interactions(train_edges, num_users, num_articles)

    def log(epoch: int, m: ImplicitALS) -> None:
        if verbose:
            r, p, n = get_metrics_lightgcn(m, val_edges, [train_edges], config.k)
            print(f"[iALS epoch {epoch + 1}/{epochs}] objective: {m.objective(inter):.6g}, val_recall@{config.k}: {r:.6f}, "
                  f"val_precision@{config.k}: {p:.6f}, val_ndcg@{config.k}: {n:.6f}")
    model.fit(inter, epochs, callback=log)
    recall, precision, _ = get_metrics_lightgcn(model, val_edges, [train_edges], config.k)
    test_recall, test_precision, test_ndcg = get_metrics_lightgcn(model, test_edges, [train_edges, val_edges], config.k)
    if verbose:
        print(f"[test_recall@{config.k}: {test_recall:.5f}, test_precision@{config.k}: {test_precision:.5f}, "
              f"test_ndcg@{config.k}: {test_ndcg:.5f}")
    if full_rank_ks is not None:
        full = evaluation_full_rank(model, test_edges, [train_edges, val_edges], tuple(full_rank_ks))
        if verbose:
            print("[test full-rank] " + ", ".join(f"{key}: {round(v, 6) if isinstance(v, float) else v}" for key, v in full.items()))
        if save_dir is not None:
            import json
            import os
            os.makedirs(save_dir, exist_ok=True)
            with open(os.path.join(save_dir, "full_rank_metrics.json"), "w") as f:
                json.dump(full, f, indent=1, sort_keys=True)
    save_predictions(model, all_edges, config.num_recommendations, save_dir)
    return Stats(loss=model.objective(inter), recall_val=recall, recall_test=test_recall, precision_val=precision,
                 precision_test=test_precision)
