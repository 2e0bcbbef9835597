"""PinSAGE evaluation — reference: pinsage/evaluation.py (LatestNNRecommender, prec, evaluate_nn) and the evaluation half of
pinsage/model.py:120-134.  The graph is the port's user -> item CSR (an AdjList, a PinSAGESampler's ui_ptr / ui_idx, or a
(ptr, idx) pair) instead of a DGL graph; the scoring is K10 (ops.topk_excl: exact top-K with per-user exclusion).
RecentItemsRecommender is the port's own: a user's last few distinct items instead of the latest one.  RandomWalkRecommender,
also the port's own, ignores the embeddings and recommends from random walks over the graph: the graph-only yardstick."""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch as t
from torch import Tensor

from .. import _lib, ops
from ..data.dataset import AdjList


def _csr(graph, device) -> Tuple[Tensor, Tensor]:
    """(ptr, idx) of a user -> item CSR as int32 tensors on `device`."""
    if hasattr(graph, "ui_ptr"):                    # PinSAGESampler: the training graph it walks
        ptr, idx = graph.ui_ptr, graph.ui_idx
    elif isinstance(graph, AdjList):
        ptr, idx = graph.ptr, graph.idx
    elif hasattr(graph, "tocsr"):                   # scipy.sparse matrix
        g = graph.tocsr()
        ptr, idx = g.indptr, g.indices
    elif isinstance(graph, (tuple, list)) and len(graph) == 2:
        ptr, idx = graph
    else:
        raise TypeError(f"a user -> item CSR is expected (AdjList, PinSAGESampler, scipy.sparse, (ptr, idx)), got {type(graph)}")
    conv = lambda a: (t.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else t.as_tensor(a))
    ptr, idx = conv(ptr), conv(idx)
    if ptr.dim() != 1 or idx.dim() != 1 or ptr.numel() < 1:
        raise ValueError("ptr and idx must be 1-D, ptr with n_users + 1 entries")
    if idx.numel() >= 2 ** 31:
        raise ValueError("more than 2^31 - 1 interactions")
    return ptr.to(device=device, dtype=t.int32).contiguous(), idx.to(device=device, dtype=t.int32).contiguous()


class LatestNNRecommender:
    """pinsage/evaluation.py:18-53: every user is represented by the item of their LATEST interaction; the K items closest to
    it by dot product, the items the user has interacted with excluded, are the recommendations.

    Latest = the LAST entry of the user's row.  Rows are kept in transaction order (data/graph_io.py:_adj_dict and AdjList
    keep list order), which stands in for the reference's dgl.sampling.select_topk(k=1, timestamp): timestamps other than
    row order are not supported.  A user without any interaction raises ValueError (the reference asserts).  Ties go to the
    lower item id; a user with fewer than K eligible items gets -1 pads (the reference would return excluded -inf items)."""

    def latest_items(self, graph, device=None) -> Tensor:
        """int64 [n_users]: the last item of every user's row."""
        return _latest(*_csr(graph, device if device is not None else _device_of(graph)))

    def recommend(self, graph, K: int, h_user: Optional[Tensor], h_item: Tensor) -> Tensor:
        """LongTensor [n_users, K] of item ids by (score desc, id asc), score = h_item[latest] . h_item[i], the user's row
        excluded.  h_user is unused (as in the reference: users are represented by their latest item)."""
        if K <= 0:
            raise ValueError("K must be positive")
        h = h_item.detach().to(t.float32).contiguous()
        ptr, idx = _csr(graph, h.device)
        latest = _latest(ptr, idx)
        excl = ops.DeviceCSR(ptr.numel() - 1, h.shape[0], ptr, idx)
        return ops.topk_excl(latest, h, h, int(K), excl)


class RecentItemsRecommender:
    """A user is represented by their last `n_recent` DISTINCT items instead of the latest one alone (the PinSAGE paper
    serves a user from several recent pins; the reference has LatestNNRecommender only).  The rule is stated step for step
    in include/laplace_hip.h ("N5 recent-items recommender") and restated in numpy by tests/recent_items_emulation.py:

      history  the last min(len, 64) entries of the user's row, most recent first; an entry whose item occurs at a more recent
               position is dropped; the first n_recent survivors are the user's slots (slot 0 = the latest item).
      weights  w[r] = float32(decay ** r): slot r counts decay ** r as much as the latest item.
      "mean"   the weighted mean of the slots' rows of h_item is the query of ONE top-K call.
      "max"    every slot retrieves its own K nearest items (LatestNNRecommender's rule applied to that slot); an item's
               score is the largest w[r] * score among the lists it appears in, and the K best by (score desc, id asc) are the
               answer.  For decay == 1 that is the exact top-K of max_r h_item[item_r] . h_item[i].

    The items of the user's whole row are excluded, ties go to the lower id, -1 pads when fewer than K items are eligible: as
    LatestNNRecommender, whose ids n_recent = 1 returns for both pools.  Recency is ROW ORDER (rows are kept in transaction
    order, the rule of this module); per-edge timestamps are not supported.  A user without any interaction raises
    ValueError.  The recommender keeps no state between calls."""

    # recommend() with pool = "max" walks the users in chunks so that the per-slot lists of a chunk — ids int64 and scores
    # float32 [n_recent, chunk, K] — stay below this many bytes whatever the number of users (8 slots at K = 10: 279 620
    # users per chunk).  The chunk's top-K workspace is ops.topk_excl's own (ops.TOPK_WS_BYTES per stream).
    MAX_LIST_BYTES = 256 << 20

    def __init__(self, n_recent: int = 8, pool: str = "max", decay: float = 1.0):
        if not isinstance(n_recent, (int, np.integer)) or not 1 <= n_recent <= _lib.MI_RECENT_MAX_SLOTS:
            raise ValueError(f"n_recent must be an integer in 1 .. {_lib.MI_RECENT_MAX_SLOTS}, got {n_recent!r}")
        if pool not in ("max", "mean"):
            raise ValueError(f"pool must be 'max' or 'mean', got {pool!r}")
        if not 0.0 < float(decay) <= 1.0:    # NaN fails both comparisons
            raise ValueError(f"decay must be in (0, 1], got {decay!r}")
        self.n_recent, self.pool, self.decay = int(n_recent), pool, float(decay)

    def weights(self) -> np.ndarray:
        """float32 [n_recent]: w[r] = (float)pow((double)decay, r)."""
        return np.array([self.decay ** r for r in range(self.n_recent)], dtype=np.float64).astype(np.float32)

    def recent_items(self, graph, device=None) -> Tuple[Tensor, Tensor]:
        """(items int64 [n_recent, n_users], n_slots int32 [n_users]): items[r] is the r-th most recent distinct item of every
        user, slots r >= n_slots[u] repeat items[0, u].  Computed on the GPU (mi_recent_items): `device`, by default the
        graph's own, must be one."""
        return self._recent(*_csr(graph, device if device is not None else _device_of(graph)))

    def _recent(self, ptr: Tensor, idx: Tensor) -> Tuple[Tensor, Tensor]:
        if bool((ptr[1:] == ptr[:-1]).any()):
            raise ValueError("every user needs at least one interaction (a user's recent items represent them)")
        return ops.recent_items(ptr, idx, self.n_recent)

    def recommend(self, graph, K: int, h_user: Optional[Tensor], h_item: Tensor, want_scores: bool = False):
        """LongTensor [n_users, K] of item ids by (score desc, id asc), the user's row excluded, -1 pads; with want_scores
        also the float32 [n_users, K] scores (-inf at pads; "mean": q . h_item[i], "max": the largest w[r] * score).  h_user
        is unused, as in LatestNNRecommender."""
        if K <= 0:
            raise ValueError("K must be positive")
        K = int(K)
        h = h_item.detach().to(t.float32).contiguous()
        ptr, idx = _csr(graph, h.device)
        items, n_slots = self._recent(ptr, idx)
        n_users = ptr.numel() - 1
        excl = ops.DeviceCSR(n_users, h.shape[0], ptr, idx)
        w = t.from_numpy(self.weights()).to(h.device)
        if self.pool == "mean":
            q = ops.pool_recent(items, n_slots, w, h)
            return ops.topk_excl(t.arange(n_users, dtype=t.int64, device=h.device), q, h, K, excl, want_scores=want_scores)
        if self.n_recent * K > _lib.MI_TOPK_MERGE_MAX_ENTRIES:
            raise ValueError(f"n_recent * K = {self.n_recent * K} is above the merge's {_lib.MI_TOPK_MERGE_MAX_ENTRIES} entries")
        chunk = max(1, min(n_users, self.MAX_LIST_BYTES // (self.n_recent * K * 12)))
        outs = []
        for u0 in range(0, n_users, chunk):
            u1 = min(n_users, u0 + chunk)
            ids = t.empty(self.n_recent, u1 - u0, K, dtype=t.int64, device=h.device)
            sc = t.empty(self.n_recent, u1 - u0, K, dtype=t.float32, device=h.device)
            ex = ops.row_slice(excl, u0, u1)    # rowptr keeps absolute offsets: a chunk's exclusion is a slice
            for r in range(self.n_recent):
                a, b = ops.topk_excl(items[r, u0:u1], h, h, K, ex, want_scores=True)
                ids[r].copy_(a)
                sc[r].copy_(b)
            outs.append(ops.topk_merge_max(ids, sc, n_slots[u0:u1], w, K, want_scores=True))
        if len(outs) == 1:
            out_ids, out_sc = outs[0]
        else:
            out_ids = t.cat([o[0] for o in outs]) if outs else t.empty(0, K, dtype=t.int64, device=h.device)
            out_sc = t.cat([o[1] for o in outs]) if outs else t.empty(0, K, dtype=t.float32, device=h.device)
        return (out_ids, out_sc) if want_scores else out_ids


class RandomWalkRecommender:
    """The graph-only yardstick of evaluate_nn: recommendations from random walks over the interaction graph alone (the
    random-walk matcher of include/laplace_hip.h, N3c, with the user's row excluded), behind LatestNNRecommender's contract.
    The embeddings are IGNORED — h_item only says how many items there are and where to compute — so
    evaluate_nn(..., recommender=RandomWalkRecommender(...)) is the hits@K a trained model has to beat on the same graph.

    The arguments are data.matching.RandomWalkMatcher's, with the same untuned defaults.  A graph that carries its item ->
    user lists (a PinSAGESampler: iu_ptr / iu_idx) is walked over them as they are; for any other form (AdjList, scipy,
    (ptr, idx)) they are derived here, the users of an item in (user id, row position) order.  Which user a draw picks
    depends on that order, so the two forms are two equally valid answers, each reproducible bit for bit."""

    def __init__(self, num_walks: int = 256, walk_length: int = 4, restart_prob: float = 0.5, n_recent: int = 8,
                 boost: str = "multi_hit", seed: int = 0):
        ops.check_random_walks(1, num_walks, walk_length, restart_prob, n_recent, boost)
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 2 ** 64:
            raise ValueError(f"seed must be an integer in [0, 2^64), got {seed!r}")
        self.num_walks, self.walk_length, self.restart_prob = int(num_walks), int(walk_length), float(restart_prob)
        self.n_recent, self.boost, self.seed = int(n_recent), boost, int(seed)

    def recommend(self, graph, K: int, h_user: Optional[Tensor], h_item: Tensor) -> Tensor:
        """LongTensor [n_users, K] of item ids by (walk score desc, id asc), the user's row excluded, -1 pads.  h_user and the
        values of h_item are unused.  A user without any interaction raises ValueError."""
        ops.check_random_walks(K, self.num_walks, self.walk_length, self.restart_prob, self.n_recent, self.boost)
        if not isinstance(h_item, Tensor) or h_item.dim() != 2:
            raise ValueError("h_item must be a [n_items, d] tensor (its rows count the items, its device is where the walks run)")
        n_items, dev = int(h_item.shape[0]), h_item.device
        ptr, idx = _csr(graph, dev)
        if bool((ptr[1:] == ptr[:-1]).any()):
            raise ValueError("every user needs at least one interaction (a user's recent items start their walks)")
        if hasattr(graph, "iu_ptr") and hasattr(graph, "iu_idx"):
            iu_ptr = t.as_tensor(graph.iu_ptr).to(device=dev, dtype=t.int32).contiguous()
            iu_idx = t.as_tensor(graph.iu_idx).to(device=dev, dtype=t.int32).contiguous()
            if iu_ptr.numel() != n_items + 1:
                raise ValueError(f"graph has {iu_ptr.numel() - 1} item rows, h_item {n_items}")
        else:
            if idx.numel() and int(idx.max()) >= n_items:
                raise ValueError(f"graph names item {int(idx.max())} but h_item has {n_items} rows")
            users = t.repeat_interleave(t.arange(ptr.numel() - 1, device=dev, dtype=t.int32), (ptr[1:] - ptr[:-1]).long())
            iu_idx = users[t.sort(idx.long(), stable=True)[1]].contiguous()
            iu_ptr = t.zeros(n_items + 1, dtype=t.int64, device=dev)
            t.cumsum(t.bincount(idx.long(), minlength=n_items), dim=0, out=iu_ptr[1:])
            iu_ptr = iu_ptr.to(t.int32)
        ids, _, _ = ops.match_random_walks(iu_ptr, iu_idx, ptr, idx, int(K), num_walks=self.num_walks,
                                           walk_length=self.walk_length, restart_prob=self.restart_prob, n_recent=self.n_recent,
                                           boost=self.boost, exclude_seen=True, seed=self.seed)
        return ids.to(t.int64)


def _latest(ptr: Tensor, idx: Tensor) -> Tensor:
    if bool((ptr[1:] == ptr[:-1]).any()):
        raise ValueError("every user needs at least one interaction (a user's latest item represents them)")
    return idx[ptr[1:].long() - 1].long()


def _device_of(graph):
    return graph.ui_ptr.device if hasattr(graph, "ui_ptr") else t.device("cpu")


def prec(recommendations: Tensor, ground_truth) -> float:
    """pinsage/evaluation.py:8-15 (hits@K): the share of ALL users with at least one of their K recommendations in their
    held-out row.  ground_truth: user -> item CSR with one row per user (scipy.sparse, AdjList, (ptr, idx)); users with no
    held-out item count as misses, -1 pads never hit.  Computed where `recommendations` lives, one host read."""
    rec = t.as_tensor(recommendations)
    if rec.dim() != 2:
        raise ValueError("recommendations must be [n_users, K]")
    dev = rec.device
    ptr, idx = _csr(ground_truth, dev)
    n_users = ptr.numel() - 1
    if n_users != rec.shape[0]:
        raise ValueError(f"ground truth has {n_users} users, recommendations {rec.shape[0]}")
    if n_users == 0:
        return 0.0
    # (user, item) -> user * 2^31 + item: held-out pairs sorted once, every recommendation looked up by binary search
    rows = t.repeat_interleave(t.arange(n_users, device=dev), (ptr[1:] - ptr[:-1]).long())
    keys = t.sort(rows * (1 << 31) + idx.long())[0]
    rec = rec.long()
    q = t.arange(n_users, device=dev)[:, None] * (1 << 31) + rec.clamp(min=0)
    pos = t.searchsorted(keys, q).clamp(max=max(keys.numel() - 1, 0))
    hit = (keys[pos] == q) & (rec >= 0) if keys.numel() else t.zeros_like(rec, dtype=t.bool)
    return float(hit.any(1).double().mean())


def evaluate_nn(model, sampler, ground_truth, K: int = 10, *, graph=None, step: Optional[int] = None, recommender=None) -> float:
    """pinsage/evaluation.py:58-72 after pinsage/model.py:120-134: every item's representation (model.item_representations),
    the recommendations over `graph` (default: the sampler's training graph) and their hits@K against `ground_truth` (the
    held-out user -> item rows).  recommender: anything with LatestNNRecommender's recommend(graph, K, h_user, h_item);
    None = LatestNNRecommender(), the reference's."""
    h_item = model.item_representations(sampler, step=step)
    rec = LatestNNRecommender() if recommender is None else recommender
    recs = rec.recommend(sampler if graph is None else graph, K, None, h_item)
    return prec(recs, ground_truth)
