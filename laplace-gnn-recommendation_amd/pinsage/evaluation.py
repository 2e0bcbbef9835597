"""PinSAGE evaluation — reference: pinsage/evaluation.py (LatestNNRecommender, prec, evaluate_nn) and the evaluation half of
pinsage/model.py:120-134.  The graph is the port's user -> item CSR (an AdjList, a PinSAGESampler's ui_ptr / ui_idx, or a
(ptr, idx) pair) instead of a DGL graph; the scoring is K10 (ops.topk_excl: exact top-K with per-user exclusion)."""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch as t
from torch import Tensor

from .. import ops
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


def evaluate_nn(model, sampler, ground_truth, K: int = 10, *, graph=None, step: Optional[int] = None) -> float:
    """pinsage/evaluation.py:58-72 after pinsage/model.py:120-134: every item's representation (model.item_representations),
    the latest-item recommendations over `graph` (default: the sampler's training graph) and their hits@K against
    `ground_truth` (the held-out user -> item rows)."""
    h_item = model.item_representations(sampler, step=step)
    recs = LatestNNRecommender().recommend(sampler if graph is None else graph, K, None, h_item)
    return prec(recs, ground_truth)
