"""Attribute node types of the ranker's batches: `Config.other_edge_types` (the reference's default dataset attaches
them to every sample, data/dataset_neo.py:67-91,140-168).

A supported relation is (article, name, T) with T a node type other than customer and article.  The full graph holds
`graph[(article, name, T)].edge_index` (int64 [2, nnz]: article id, T id; any order, duplicates dropped) and
`graph[T].x` ([n_T, F_T]).  The one rule, for the host dataset and the device sampler alike — per sample, whose
articles are a_0 < ... < a_{m-1} at local indices 0..m-1:

    T nodes   the sorted distinct ids of the union of rel[a_j];  x = graph[T].x[ids], n_id = ids
    edges     for j ascending and, within j, e in rel[a_j] ascending: (j, rank of e among the T nodes)
    stores    (article, name, T).edge_index and (T, "rev_" + name, article).edge_index = its flip; no edge_label*

All articles of the sample take part, label articles included, in train and in evaluation mode.  Attribute nodes are
never expanded into further articles (a colour group holds thousands of them): DESIGN section 6.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Tuple

import numpy as np
import torch as t
from torch import Tensor

from ..hetero import HeteroData
from ..utils.constants import Constants


@dataclass
class Relation:
    key: Tuple[str, str, str]       # (article, name, T)
    rev_key: Tuple[str, str, str]   # (T, "rev_" + name, article)
    target: str
    ptr: np.ndarray                 # int64[num_articles + 1]
    idx: np.ndarray                 # int64[nnz], every row strictly ascending
    n_targets: int
    x: Tensor                       # graph[T].x

    def rows(self, articles: np.ndarray):
        """(the rows of `articles` one after the other, their lengths)."""
        cnt = self.ptr[articles + 1] - self.ptr[articles]
        total = int(cnt.sum())
        if total == 0:
            return np.empty(0, dtype=np.int64), cnt
        start = np.repeat(self.ptr[articles], cnt)
        within = np.arange(total) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        return self.idx[start + within], cnt


def resolve_relations(config, graph: HeteroData) -> List[Relation]:
    """The relations of `config.other_edge_types` as CSRs over the articles of `graph`; [] when there are none.
    ValueError for an entry of another shape, a target type that `config.node_types` or the graph does not hold, or
    ids outside the node tables."""
    entries = list(getattr(config, "other_edge_types", None) or [])
    if not entries:
        return []
    n_articles = int(graph[Constants.node_item].x.shape[0])
    declared = list(getattr(config, "node_types", None) or [])
    out: List[Relation] = []
    for entry in entries:
        ok = (isinstance(entry, (tuple, list)) and len(entry) == 3 and all(isinstance(p, str) for p in entry)
              and entry[0] == Constants.node_item and entry[2] not in (Constants.node_user, Constants.node_item))
        if not ok:
            raise ValueError(f"other_edge_types entry {entry!r}: only ({Constants.node_item!r}, name, T) with T a node type "
                             f"other than {Constants.node_user!r} and {Constants.node_item!r} is supported")
        key = tuple(entry)
        _, name, target = key
        if target not in declared:
            raise ValueError(f"other_edge_types entry {entry!r}: node type {target!r} is not in config.node_types")
        if target not in graph.node_types or "x" not in graph[target]:
            raise ValueError(f"other_edge_types entry {entry!r}: the graph holds no features for node type {target!r}")
        if key not in graph.edge_types or "edge_index" not in graph[key]:
            raise ValueError(f"other_edge_types entry {entry!r}: the graph holds no edge_index for this relation")
        if any(r.target == target for r in out):
            raise ValueError(f"other_edge_types entry {entry!r}: node type {target!r} already has a relation")
        x = graph[target].x
        n_targets = int(x.shape[0])
        ei = graph[key].edge_index
        ei = (ei.detach().cpu().numpy() if isinstance(ei, Tensor) else np.asarray(ei)).astype(np.int64).reshape(2, -1)
        if n_targets < 1 or n_targets >= 2**31 or ei.shape[1] >= 2**31:
            raise ValueError(f"other_edge_types entry {entry!r}: {n_targets} target nodes / {ei.shape[1]} edges")
        if ei.shape[1] and (ei[0].min() < 0 or ei[0].max() >= n_articles or ei[1].min() < 0 or ei[1].max() >= n_targets):
            raise ValueError(f"other_edge_types entry {entry!r}: edge_index has ids outside [0, {n_articles}) x [0, {n_targets})")
        pairs = np.unique(ei[0] * n_targets + ei[1])           # sorted by (article, target), duplicates dropped
        src, idx = pairs // n_targets, pairs % n_targets
        ptr = np.zeros(n_articles + 1, dtype=np.int64)
        np.cumsum(np.bincount(src, minlength=n_articles), out=ptr[1:])
        out.append(Relation(key, (target, "rev_" + name, Constants.node_item), target, ptr, idx.astype(np.int64), n_targets, x))
    return out


def attach_relations(data: HeteroData, relations: List[Relation], article_ids: np.ndarray) -> HeteroData:
    """The host form of the rule for one sample whose articles (sorted global ids) are `article_ids`."""
    for rel in relations:
        flat, cnt = rel.rows(article_ids)
        t_ids = np.unique(flat)
        ids = t.from_numpy(t_ids)
        data[rel.target].x = rel.x[ids]
        data[rel.target].n_id = ids
        edge_index = t.from_numpy(np.stack([np.repeat(np.arange(article_ids.shape[0], dtype=np.int64), cnt),
                                            np.searchsorted(t_ids, flat).astype(np.int64)]))
        data[rel.key].edge_index = edge_index
        data[rel.rev_key].edge_index = edge_index.flip(0)
    return data
