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

Not built: frequency-scaled regularisation, per-edge confidences, the CG solver, the paper's block-outer schedule of iALS++
(all rows inside one block step, predictions of all pairs kept between steps), hub rows split over workgroups, dim > 256, a
sharded form, bf16, and the matcher's entry in get_matchers / tools/e2e_hm_scale.py's chain.
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


class ImplicitALS(t.nn.Module):
    """iALS with confidence 1 + alpha on the observed pairs and 1 on all others, L2 weight reg on both tables.  A pair that
    occurs twice in `interactions` counts twice (the kernel sums a row's entries as written); the pipeline's graphs are
    deduplicated."""

    def __init__(self, num_users: int, num_items: int, dim: int = 64, alpha: float = 1.0, reg: float = 20.0, seed: int = 0,
                 init_std: float = 0.1, solver: str = "cholesky", block: int = 16, block_sweeps: int = 1,
                 fold_in_sweeps: int = 4):
        super().__init__()
        if solver not in SOLVERS:
            raise ValueError(f"solver must be one of {SOLVERS}, got {solver!r}")
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

    # ---- the graph -----------------------------------------------------------------------------------------------------
    def bind(self, interactions: Interactions) -> None:
        """The training graph of the half-sweeps that follow: its users x items CSR and, built once, the transposed one."""
        if self._bound is not None and self._bound[0] is interactions:
            return
        if interactions.num_users != self.num_users or interactions.num_items != self.num_items:
            raise ValueError(f"interactions are {interactions.num_users} x {interactions.num_items}, the model "
                             f"{self.num_users} x {self.num_items}")
        inter = interactions.to(self.items_emb.weight.device)
        by_user = inter.csr()
        self._bound = (interactions, by_user, ops.csr_transpose(by_user))

    def _tables(self, side: str) -> Tuple[Tensor, Tensor]:
        if side not in SIDES:
            raise ValueError(f"side must be one of {SIDES}, got {side!r}")
        mine, other = (self.users_emb, self.items_emb) if side == "users" else (self.items_emb, self.users_emb)
        return mine.weight.data, other.weight.data

    def _solve(self, csr: ops.DeviceCSR, fixed: Tensor, out: Optional[Tensor]) -> Tuple[Tensor, Tensor]:
        """`out` is the table of a half-sweep (the block solver's start as well) or None for a fold-in (a zero start)."""
        gram = ops.gemm(fixed, fixed, trans_a=True, trans_b=False)
        if self.solver == "block":
            return ops.als_block_rows(csr, fixed, gram, alpha=self.alpha, reg=self.reg, block=self.block, x=out,
                                      sweeps=self.block_sweeps if out is not None else self.fold_in_sweeps)
        return ops.als_solve_rows(csr, fixed, gram, alpha=self.alpha, reg=self.reg, out=out)

    def half_sweep(self, side: str, interactions: Optional[Interactions] = None) -> Tensor:
        """Re-solves every row of one table against the other.  Returns the device counter of rows whose factorisation
        failed (int32 [1]; those rows are zero) without reading it: fit() reads it once per epoch."""
        if interactions is not None:
            self.bind(interactions)
        if self._bound is None:
            raise RuntimeError("half_sweep needs a graph: pass interactions, or call bind() / fit() first")
        mine, other = self._tables(side)
        csr = self._bound[1] if side == "users" else self._bound[2]
        return self._solve(csr, other, mine)[1]

    def fit(self, interactions: Interactions, epochs: int, callback: Optional[Callable[[int, "ImplicitALS"], None]] = None
            ) -> "ImplicitALS":
        """`epochs` times a user half-sweep, then an item half-sweep.  callback(epoch, model) runs after each epoch."""
        self.bind(interactions)
        for epoch in range(int(epochs)):
            failed = self.half_sweep("users") + self.half_sweep("items")
            n = int(failed.item())   # the epoch's one read-back
            if n:
                raise RuntimeError(f"iALS epoch {epoch}: {n} row systems met a non-positive or non-finite pivot "
                                   f"(alpha={self.alpha}, reg={self.reg}); the rows were zeroed")
            if callback is not None:
                callback(epoch, self)
        return self

    def fold_in(self, ptr: Tensor, idx: Tensor) -> Tensor:
        """Vectors [len(ptr) - 1, dim] for rows that are not in the model — an int32 CSR (ptr, idx) over ITEM ids — against
        the current item table: a user half-sweep on another CSR, so a new interaction is seen at once.  The block solver
        starts these rows from zero and makes fold_in_sweeps passes over them."""
        csr = ops.DeviceCSR(int(ptr.numel()) - 1, self.num_items, ptr, idx)
        x, failed = self._solve(csr, self.items_emb.weight.data, None)
        n = int(failed.item())
        if n:
            raise RuntimeError(f"iALS fold-in: {n} row systems met a non-positive or non-finite pivot")
        return x

    # ---- for tests and logs ----------------------------------------------------------------------------------------------
    def objective(self, interactions: Interactions, edge_block: int = 1 << 20) -> float:
        """The iALS objective, halved so that a row's share is 1/2 x^T A x - b^T x + const with the A and b of the rule:
            1/2 * sum over ALL (u, i) of c_ui (p_ui - x_u . y_i)^2  +  reg / 2 * (|X|_F^2 + |Y|_F^2),
        c = 1 + alpha, p = 1 on the observed pairs (every occurrence of a repeated pair), c = 1, p = 0 elsewhere.  float64
        torch on the device, through the Gram matrix: not on the hot path."""
        X = self.users_emb.weight.data.double()
        Y = self.items_emb.weight.data.double()
        ei = interactions.edge_index.to(X.device)
        total = ((X @ (Y.T @ Y)) * X).sum()   # sum over all pairs of (x . y)^2
        for e0 in range(0, ei.shape[1], edge_block):
            u, i = ei[0, e0:e0 + edge_block], ei[1, e0:e0 + edge_block]
            s = (X[u] * Y[i]).sum(dim=1)
            total = total + ((1.0 + self.alpha) * (1.0 - s) ** 2 - s * s).sum()
        total = total + self.reg * ((X * X).sum() + (Y * Y).sum())
        return 0.5 * float(total)


def train(config, *, edge_index: Tensor, num_users: int, num_articles: int, dim: int = 64, alpha: float = 1.0,
          reg: float = 20.0, epochs: int = 3, seed: int = 0, device: str = "cuda", save_dir: Optional[str] = None,
          full_rank_ks: Optional[Tuple[int, ...]] = (12, 100), verbose: bool = True, solver: str = "cholesky",
          block: int = 16, block_sweeps: int = 1) -> Stats:
    """run_pipeline_lightgcn.train with iALS in the trainer's place: the same split (create_dataloaders_lightgcn), the ranking
    metrics @ config.k on validation and test, evaluation_full_rank on the test split and save_predictions — the same three
    files (lightgcn_output.pt and the two tables) that data.matching.LightGCNMatcher consumes.  Stats.loss is the objective
    on the training edges."""
    from .data.lightgcn_loader import create_dataloaders_lightgcn
    from .run_pipeline_lightgcn import evaluation_full_rank, save_predictions
    from .utils.metrics_lightgcn import get_metrics_lightgcn
    (_, _, _, train_edges, val_edges, test_edges, all_edges, num_users,
     num_articles) = create_dataloaders_lightgcn(edge_index, num_users, num_articles, compat="bipartite", device=device)
    model = ImplicitALS(num_users, num_articles, dim=dim, alpha=alpha, reg=reg, seed=seed, solver=solver, block=block,
                        block_sweeps=block_sweeps).to(device)
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
