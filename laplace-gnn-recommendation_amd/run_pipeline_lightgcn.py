"""LightGCN candidate-generation pipeline — the loop of the reference's run_pipeline_lightgcn.py
(evaluation(): 20-73, train(): 76-232) with every stage on the GPU.

Differences a caller sees: the graph is passed in (edge_index + node counts) instead of being
unpickled from PyG files, and the top-`num_recommendations` dump is returned as one [U, k] tensor
(optionally saved) instead of a dict of per-user tensors built in a Python loop.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch as t
from torch import Tensor

from . import ops
from .config import LightGCNConfig, lightgcn_config
from .data.lightgcn_loader import create_dataloaders_lightgcn
from .interactions import Interactions
from .model.lightgcn import LightGCN
from .reporting.types import Stats
from .sparse import SparseTensor
from .trainer import LightGCNTrainer
from .utils.metrics_lightgcn import get_full_rank_metrics_lightgcn, get_metrics_lightgcn, topk_for_users


PREDICTORS = ("layer0", "propagated")


def propagated_embeddings(model: LightGCN, train_sparse: SparseTensor) -> Tuple[Tensor, Tensor]:
    """(users, items) rows of mean_k(A^k E0) on the TRAINING adjacency: what the loss trains."""
    with t.no_grad():
        users_final, _, items_final, _ = model.forward(train_sparse)
    return users_final.contiguous(), items_final.contiguous()


def evaluation(model: LightGCN, edge_index: Tensor, sparse_edge_index: SparseTensor,
               exclude_edge_indices: List[Tensor], k: int, lambda_val: float, seed: int = 0, *,
               objective: str = "reference", embeddings: Optional[Tuple[Tensor, Tensor]] = None
               ) -> Tuple[float, float, float, float]:
    """loss over every edge of the split (one structured negative each) on the split's own
    adjacency, plus recall / precision / ndcg @ k (run_pipeline_lightgcn.py:20-73).  objective: the loss's form
    (default: the reference's); embeddings: the tables the ranking metrics score with (default: layer 0).
    The negatives are uniform and the loss carries no logQ correction whatever sampler the training run used."""
    with t.no_grad():
        users_final, users_0, items_final, items_0 = model.forward(sparse_edge_index)
        n_users, n_items = model.num_users, model.num_items
        inter = Interactions(edge_index, n_users, n_items)
        neg_range = int(edge_index[1].max())  # reference: num_nodes = max(edge_index[1])
        u, p, n = ops.sample_bpr_batch(inter.csr(), inter.row_of_edge(), inter.num_edges, neg_range, seed, 0,
                                       quirk=True, edges_in_order=True, no_self_loops=True)  # :40-44 contains_neg_self_loops=False
        final = t.cat([users_final, items_final])
        loss = ops.rank_loss_fwd_bwd(u, p, n, final, model.table(), n_users, lambda_val, objective=objective)
    recall, precision, ndcg = get_metrics_lightgcn(model, edge_index, exclude_edge_indices, k, embeddings=embeddings)
    return float(loss), recall, precision, ndcg


def evaluation_full_rank(model: LightGCN, edge_index: Tensor, exclude_edge_indices: List[Tensor], ks=(12,),
                         embeddings: Optional[Tuple[Tensor, Tensor]] = None, filtered: bool = False) -> dict:
    """The split's metrics from the full-catalogue rank of every held-out pair (utils.metrics_lightgcn.full_rank_metrics):
    recall / precision / ndcg / map @ every K of `ks`, mrr, mean_rank, auc.  The float entries only: what a log line or a
    JSON file holds.  Same tables and exclusions as evaluation()'s ranking metrics, so recall@k is evaluation()'s recall."""
    m = get_full_rank_metrics_lightgcn(model, edge_index, exclude_edge_indices, ks, embeddings=embeddings, filtered=filtered)
    return {key: v for key, v in m.items() if not isinstance(v, Tensor)}


def train(config: LightGCNConfig = lightgcn_config, *, edge_index: Tensor, num_users: int, num_articles: int,
          compat: str = "reference", device: str = "cuda", seed: int = 0, save_dir: Optional[str] = None,
          verbose: bool = True, objective: str = "reference", n_neg: int = 1, predictor: str = "layer0",
          negatives: str = "uniform", neg_power: float = 0.75, in_batch_group: int = 1024,
          full_rank_ks: Optional[Tuple[int, ...]] = None, full_softmax: bool = False, cl_weight: float = 0.0,
          cl_eps: float = 0.2, cl_tau: float = 0.15, cl_layer: int = 1, cl_group: int = 1024,
          layer_dtype: str = "f32") -> Stats:
    """objective / n_neg: the training loss (trainer.LightGCNTrainer).  predictor="propagated": evaluation,
    the ranking metrics and the saved predictions score with mean_k(A^k E0) of the training adjacency — the scores the
    loss trains — instead of the layer-0 tables.
    negatives="popularity": training negatives drawn ∝ (training degree) ** neg_power over every item, with the logQ
    correction when objective == "softmax"; the reference's negative range and sampler quirk do not apply to that
    sampler and are left out.  negatives="in_batch" (objective="softmax"): the other positives of a slot's group of
    in_batch_group slots are its negatives, logQ-corrected by training degree; likewise without the reference's range and
    quirk.  full_softmax=True (objective="softmax", negatives="uniform"): the exact softmax over every item, in the dense
    step form (sparse_batch=False is chosen here), also without the range and the quirk.
    cl_weight > 0: the noise-view contrastive term (LightGCNTrainer's cl_* keywords, passed through) is added to the training
    loss, in the dense step form (chosen here as well).
    layer_dtype="bf16": the training step keeps the layers of its forward in bf16 (LightGCNTrainer's keyword, passed through);
    evaluation and the saved predictions keep the f32 forward.
    evaluation() keeps its uniform negatives and uncorrected loss in every case, so
    validation and test losses stay comparable across samplers.
    full_rank_ks: when given, the test split is also scored by evaluation_full_rank at these K (same predictor, same
    exclusions); the dict is printed under `verbose` and, with `save_dir`, written as full_rank_metrics.json.  The returned
    Stats are the same either way."""
    if predictor not in PREDICTORS:
        raise ValueError(f"predictor must be one of {PREDICTORS}, got {predictor!r}")
    if verbose:
        config.print()
    (train_sparse, val_sparse, test_sparse, train_edges, val_edges, test_edges, all_edges, num_users,
     num_articles) = create_dataloaders_lightgcn(edge_index, num_users, num_articles, compat=compat, device=device)

    t.manual_seed(seed)
    model = LightGCN(num_users, num_articles, embedding_dim=config.hidden_layer_size,
                     num_iterations=config.num_iterations).to(device)
    model.train()
    train_inter = Interactions(train_edges, num_users, num_articles)
    # reference sampler: negatives from [0, max train item id) with its key-collision quirk
    # samplers over every item (or no sampler at all), without the reference's quirk
    popular = negatives in ("popularity", "in_batch") or full_softmax
    exact = dict(full_softmax=True, sparse_batch=False) if full_softmax else {}
    if cl_weight:
        exact.update(sparse_batch=False, cl_weight=cl_weight, cl_eps=cl_eps, cl_tau=cl_tau, cl_layer=cl_layer, cl_group=cl_group)
    trainer = LightGCNTrainer(model, train_sparse, train_inter, lr=config.learning_rate, Lambda=config.Lambda,
                              batch_size=config.batch_size, seed=seed,
                              neg_range=None if popular else int(train_edges[1].max()),
                              reference_sampler_quirks=(compat == "reference" and not popular), objective=objective,
                              n_neg=n_neg, negatives=negatives, neg_power=neg_power, in_batch_group=in_batch_group,
                              layer_dtype=layer_dtype, **exact)

    def scoring_tables():
        return propagated_embeddings(model, train_sparse) if predictor == "propagated" else None
    train_loss = t.zeros(1, device=device)
    recall = precision = 0.0
    try:   # the trainer permutes the model's rows in place: whatever happens, hand them back under their original ids
        for it in range(config.epochs):
            train_loss = trainer.step()
            if it % config.eval_every == 0:
                model.eval()
                trainer.to_original_order()  # evaluation reads the model's tables by original id; step() re-enters the training order
                val_loss, recall, precision, ndcg = evaluation(model, val_edges, val_sparse, [train_edges], config.k,
                                                               config.Lambda, seed, objective=objective,
                                                               embeddings=scoring_tables())
                if verbose:
                    print(f"[Iter {it}/{config.epochs}] train_loss: {round(float(train_loss), 5)}, val_loss: "
                          f"{round(val_loss, 5)}, val_recall@{config.k}: {round(recall, 6)}, val_precision@{config.k}: "
                          f"{round(precision, 6)}, val_ndcg@{config.k}: {round(ndcg, 6)}")
                model.train()
            if it % config.lr_decay_every == 0 and it != 0:
                trainer.decay_lr(0.95)
    finally:
        trainer.finish()

    model.eval()
    test_loss, test_recall, test_precision, test_ndcg = evaluation(
        model, test_edges, test_sparse, [train_edges, val_edges], config.k, config.Lambda, seed, objective=objective,
        embeddings=scoring_tables())
    if verbose:
        print(f"[test_loss: {round(test_loss, 5)}, test_recall@{config.k}: {round(test_recall, 5)}, "
              f"test_precision@{config.k}: {round(test_precision, 5)}, test_ndcg@{config.k}: {round(test_ndcg, 5)}")
    if full_rank_ks is not None:
        full = evaluation_full_rank(model, test_edges, [train_edges, val_edges], tuple(full_rank_ks),
                                    embeddings=scoring_tables())
        if verbose:
            print("[test full-rank] " + ", ".join(f"{key}: {round(v, 6) if isinstance(v, float) else v}" for key, v in full.items()))
        if save_dir is not None:
            import json
            import os
            os.makedirs(save_dir, exist_ok=True)
            with open(os.path.join(save_dir, "full_rank_metrics.json"), "w") as f:
                json.dump(full, f, indent=1, sort_keys=True)

    # predictions for the matcher: top `num_recommendations` unseen items per user, layer-0 scores (F8) by default
    top_items = save_predictions(model, all_edges, config.num_recommendations, save_dir, embeddings=scoring_tables())
    return Stats(loss=float(train_loss), recall_val=recall, recall_test=test_recall, precision_val=precision,
                 precision_test=test_precision)


def save_predictions(model: LightGCN, all_edges: Tensor, num_recommendations: int,
                     save_dir: Optional[str] = None, embeddings: Optional[Tuple[Tensor, Tensor]] = None) -> Tensor:
    """[U, num_recommendations] item ids (run_pipeline_lightgcn.py:210-238); embeddings = (users, items) tables to
    score and dump instead of the layer-0 ones."""
    k = min(num_recommendations, model.num_items)
    users = t.arange(model.num_users, dtype=t.int64, device=all_edges.device)
    ue, ie = embeddings if embeddings is not None else (model.users_emb.weight.detach(), model.items_emb.weight.detach())
    top = topk_for_users(ue, ie, users, all_edges, k)
    if save_dir is not None:
        import os
        os.makedirs(save_dir, exist_ok=True)
        t.save(top.cpu(), os.path.join(save_dir, "lightgcn_output.pt"))
        t.save(ue.cpu(), os.path.join(save_dir, "users_emb_final_lightgcn.pt"))
        t.save(ie.cpu(), os.path.join(save_dir, "items_emb_final_lightgcn.pt"))
    return top
