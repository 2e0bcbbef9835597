"""LightGCN loss / evaluation helpers with the reference's call signatures
(utils/metrics_lightgcn.py), running on the HIP kernels.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch as t
from torch import Tensor

from .. import ops


class _BprLossFn(t.autograd.Function):
    """bpr_loss over six already-gathered [B, D] blocks through mi_bpr_fwd_bwd_f32.

    The blocks are laid out as two 3B-row tables (final | layer-0) and addressed by arange, so the
    same fused kernel serves this drop-in signature and the trainer's index-based fast path.
    """

    @staticmethod
    def forward(ctx, uf, u0, pf, p0, nf, n0, lambda_val: float):
        B, _ = uf.shape
        final = t.cat([uf, pf, nf]).contiguous()
        e0 = t.cat([u0, p0, n0]).contiguous()
        dev = uf.device
        users = t.arange(B, device=dev)
        neg = t.arange(B, 2 * B, device=dev)
        g_final = t.zeros_like(final)
        reg_w = t.zeros(3 * B, device=dev)
        loss = ops.bpr_fwd_bwd(users, users, neg, final, e0, B, lambda_val, g_final=g_final, reg_w=reg_w)
        ctx.save_for_backward(g_final, reg_w, e0)
        ctx.B = B
        return loss.reshape(())

    @staticmethod
    def backward(ctx, grad_out):
        g_final, reg_w, e0 = ctx.saved_tensors
        B = ctx.B
        gf = g_final * grad_out
        g0 = (reg_w[:, None] * e0) * grad_out
        return gf[:B], g0[:B], gf[B:2 * B], g0[B:2 * B], gf[2 * B:], g0[2 * B:], None


def bpr_loss(users_emb_final: Tensor, users_emb_0: Tensor, pos_items_emb_final: Tensor, pos_items_emb_0: Tensor,
             neg_items_emb_final: Tensor, neg_items_emb_0: Tensor, lambda_val: float) -> Tensor:
    """-mean(softplus(pos - neg)) + lambda * (|u0|^2 + |p0|^2 + |n0|^2), as written in the reference
    (utils/metrics_lightgcn.py:9-45; note the sign convention)."""
    return _BprLossFn.apply(users_emb_final, users_emb_0, pos_items_emb_final, pos_items_emb_0,
                            neg_items_emb_final, neg_items_emb_0, float(lambda_val))


class _RankingLossFn(t.autograd.Function):
    """ranking_loss over gathered blocks through mi_rank_loss_fwd_bwd_f32: the blocks become two (2 + M) B-row tables
    (users | positives | negatives, slot-major) addressed by arange, as in _BprLossFn."""

    @staticmethod
    def forward(ctx, uf, u0, pf, p0, nf, n0, lambda_val: float, objective: str, logq: Optional[Tensor] = None):
        B, D = uf.shape
        M = nf.shape[1]
        final = t.cat([uf, pf, nf.reshape(B * M, D)]).contiguous()
        e0 = t.cat([u0, p0, n0.reshape(B * M, D)]).contiguous()
        dev = uf.device
        users = t.arange(B, device=dev)
        neg = t.arange(B, B + B * M, device=dev).reshape(B, M)   # item ids: the positives are items [0, B)
        g_final = t.zeros_like(final)
        reg_w = t.zeros((2 + M) * B, device=dev)
        loss = ops.rank_loss_fwd_bwd(users, users, neg, final, e0, B, lambda_val, objective=objective, g_final=g_final,
                                     reg_w=reg_w, logq=logq)
        ctx.save_for_backward(g_final, reg_w, e0)
        ctx.dims = (B, M, D)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, grad_out):
        g_final, reg_w, e0 = ctx.saved_tensors
        B, M, D = ctx.dims
        gf = g_final * grad_out
        g0 = (reg_w[:, None] * e0) * grad_out
        return (gf[:B], g0[:B], gf[B:2 * B], g0[B:2 * B], gf[2 * B:].reshape(B, M, D), g0[2 * B:].reshape(B, M, D),
                None, None, None)


def ranking_loss(users_emb_final: Tensor, users_emb_0: Tensor, pos_items_emb_final: Tensor, pos_items_emb_0: Tensor,
                 neg_items_emb_final: Tensor, neg_items_emb_0: Tensor, lambda_val: float,
                 objective: str = "reference", logq: Optional[Tuple[Tensor, Tensor]] = None) -> Tensor:
    """bpr_loss with a choice of objective and M negatives per positive (negatives [B, D] or [B, M, D], M <= 16):
    "reference" -mean softplus(x) as the reference writes it, "bpr" -mean log sigmoid(x), "softmax" the sampled softmax
    over (positive, negatives); x = <u, p> - <u, n>.  The L2 term is the reference's sum form over all 2 + M rows.
    logq = (pos_logq [B], neg_logq [B] or [B, M]), float32 constants (no gradient): the softmax's logits become
    <u, p> - pos_logq and <u, n> - neg_logq, the logQ correction of negatives drawn from a proposal q."""
    ops.rank_objective_code(objective)
    if logq is not None and objective != "softmax":
        raise ValueError(f"logq corrects the sampled softmax only, not objective={objective!r}")
    if neg_items_emb_final.dim() not in (2, 3) or neg_items_emb_0.shape != neg_items_emb_final.shape:
        raise ValueError("negatives: [B, D] or [B, M, D], the same shape for both tables")
    two_d = neg_items_emb_final.dim() == 2
    nf = neg_items_emb_final[:, None, :] if two_d else neg_items_emb_final
    n0 = neg_items_emb_0[:, None, :] if two_d else neg_items_emb_0
    ops.check_n_neg(int(nf.shape[1]))
    if logq is None:
        return _RankingLossFn.apply(users_emb_final, users_emb_0, pos_items_emb_final, pos_items_emb_0, nf, n0,
                                    float(lambda_val), objective)
    pos_logq, neg_logq = logq
    B, M = int(nf.shape[0]), int(nf.shape[1])
    if pos_logq.numel() != B or neg_logq.numel() != B * M:
        raise ValueError(f"logq: pos_logq [{B}] and neg_logq [{B}, {M}] expected")
    # the position-addressed table of _RankingLossFn: positives are items [0, B), negative (b, m) is item B + b M + m
    table = t.cat([pos_logq.detach().reshape(B), neg_logq.detach().reshape(B * M)]).to(t.float32).contiguous()
    return _RankingLossFn.apply(users_emb_final, users_emb_0, pos_items_emb_final, pos_items_emb_0, nf, n0,
                                float(lambda_val), objective, table)


class _InBatchSoftmaxFn(t.autograd.Function):
    """in_batch_softmax_loss over gathered blocks through mi_inbatch_softmax_fwd_bwd_f32.  The entry knows a slot's user
    and item by the row it reads, so the blocks become one table row per DISTINCT id (the block row of the id's first
    slot); the gradient of an id comes back whole at that slot and zero at its other slots, which is what the backward of
    the gather that made the blocks adds up."""

    @staticmethod
    def forward(ctx, uf, u0, pf, p0, lambda_val: float, uinv, ufirst, iinv, ifirst, logq, group: int):
        B = uf.shape[0]
        nu = ufirst.numel()
        final = t.cat([uf[ufirst], pf[ifirst]]).contiguous()
        e0 = t.cat([u0[ufirst], p0[ifirst]]).contiguous()
        table = None if logq is None else logq.detach().reshape(B).to(t.float32)[ifirst].contiguous()
        g_final = t.zeros_like(final)
        reg_w = t.zeros(final.shape[0], device=uf.device)
        loss = ops.inbatch_softmax_fwd_bwd(uinv, iinv, final, e0, nu, lambda_val, group=group, logq=table,
                                           g_final=g_final, reg_w=reg_w)
        ctx.save_for_backward(g_final, reg_w, e0, ufirst, ifirst)
        ctx.B = B
        return loss.reshape(())

    @staticmethod
    def backward(ctx, grad_out):
        g_final, reg_w, e0, ufirst, ifirst = ctx.saved_tensors
        B, nu = ctx.B, ufirst.numel()
        gf = g_final * grad_out
        g0 = (reg_w[:, None] * e0) * grad_out
        outs = []
        for g, first in ((gf[:nu], ufirst), (g0[:nu], ufirst), (gf[nu:], ifirst), (g0[nu:], ifirst)):
            full = g.new_zeros(B, g.shape[1])
            full[first] = g
            outs.append(full)
        return (*outs, None, None, None, None, None, None, None)


def _first_slots(ids: Optional[Tensor], B: int, device):
    """(inverse [B], first [n_distinct]): the distinct-id number of every slot and the first slot of every distinct id."""
    if ids is None:
        a = t.arange(B, device=device)
        return a, a
    if ids.numel() != B:
        raise ValueError(f"ids: one per slot expected ({B}), got {ids.numel()}")
    uniq, inv = t.unique(ids.reshape(B), return_inverse=True)
    first = t.full((uniq.numel(),), B, dtype=t.int64, device=ids.device)
    first.scatter_reduce_(0, inv, t.arange(B, device=ids.device), reduce="amin")
    return inv.contiguous(), first


def in_batch_softmax_loss(users_emb_final: Tensor, users_emb_0: Tensor, pos_items_emb_final: Tensor, pos_items_emb_0: Tensor,
                          lambda_val: float, *, user_ids: Optional[Tensor] = None, item_ids: Optional[Tensor] = None,
                          logq: Optional[Tensor] = None, group: int = 1024) -> Tensor:
    """The sampled softmax with in-batch negatives: slot b's candidates are the positives of its group of `group`
    consecutive slots, with the logit <u_b, p_j> - logq[j]; a candidate with slot b's item id or slot b's user id is left out
    (ids default to arange: no masks).  The user's other items that happen to be in the group are not rejected — the usual
    approximation.  logq [B]: log-probability of each slot's positive under the batch's proposal (float32 constants).
    Slots with equal ids must carry equal rows (blocks gathered from one table)."""
    ops.check_inbatch_group(group)
    B = int(users_emb_final.shape[0])
    if logq is not None and logq.numel() != B:
        raise ValueError(f"logq: [{B}] expected, got {tuple(logq.shape)}")
    dev = users_emb_final.device
    uinv, ufirst = _first_slots(user_ids, B, dev)
    iinv, ifirst = _first_slots(item_ids, B, dev)
    return _InBatchSoftmaxFn.apply(users_emb_final, users_emb_0, pos_items_emb_final, pos_items_emb_0, float(lambda_val),
                                   uinv, ufirst, iinv, ifirst, logq, group)


class _ContrastiveFn(t.autograd.Function):
    """contrastive_loss over gathered blocks through mi_contrastive_fwd_bwd_f32.  The entry knows a slot's node by the row
    it reads, so the blocks become one table row per DISTINCT id, as in _InBatchSoftmaxFn: the gradient of an id comes back
    whole at its first slot and zero at its other slots."""

    @staticmethod
    def forward(ctx, f_rows, x_rows, inv, first, tau: float, group: int):
        a, b = f_rows[first].contiguous(), x_rows[first].contiguous()
        g_a, g_b = t.zeros_like(a), t.zeros_like(b)
        loss = ops.contrastive_fwd_bwd(inv, a, b, tau=tau, group=group, g_a=g_a, g_b=g_b)
        ctx.save_for_backward(g_a, g_b, first)
        ctx.B = f_rows.shape[0]
        return loss.reshape(())

    @staticmethod
    def backward(ctx, grad_out):
        g_a, g_b, first = ctx.saved_tensors
        outs = []
        for g in (g_a, g_b):
            full = g.new_zeros(ctx.B, g.shape[1])
            full[first] = g * grad_out
            outs.append(full)
        return (*outs, None, None, None, None)


def contrastive_loss(f_rows: Tensor, x_rows: Tensor, ids: Optional[Tensor], tau: float, group: int = 1024) -> Tensor:
    """The noise-view contrastive term over gathered blocks: InfoNCE between the normalised rows f_rows[b] (the final
    read-out of slot b's node) and x_rows[j] (layer l* of slot j's node) over groups of `group` consecutive slots at
    temperature tau; another slot with slot b's id is left out of b's candidates (ids None: arange, no masks).  Slots with
    equal ids must carry equal rows (blocks gathered from one table).  The rule is in include/laplace_hip.h."""
    B = int(f_rows.shape[0])
    if x_rows.shape != f_rows.shape:
        raise ValueError(f"x_rows: shape {tuple(f_rows.shape)} expected, got {tuple(x_rows.shape)}")
    ops.check_contrastive(int(f_rows.shape[1]), tau=tau, group=group)
    inv, first = _first_slots(ids, B, f_rows.device)
    return _ContrastiveFn.apply(f_rows, x_rows, inv, first, float(tau), group)


class _FullSoftmaxFn(t.autograd.Function):
    """full_softmax_loss through mi_full_softmax_fwd_bwd_f32: the user block and the item table become one table whose user
    rows are the B slots (slot b is user b), and the positives' layer-0 rows go to their items' rows of a layer-0 table."""

    @staticmethod
    def forward(ctx, uf, itf, pos, u0, p0, lambda_val: float):
        B, n_items = uf.shape[0], itf.shape[0]
        final = t.cat([uf, itf]).contiguous()
        e0 = t.cat([u0, u0.new_zeros(n_items, u0.shape[1])])
        e0[B + pos] = p0                     # slots with equal ids carry equal rows
        g_final = t.zeros_like(final)
        loss = ops.full_softmax_fwd_bwd(t.arange(B, device=uf.device), pos, final, e0, B, lambda_val, g_final=g_final)
        ctx.save_for_backward(g_final, u0, p0)
        ctx.B, ctx.lam = B, lambda_val
        return loss.reshape(())

    @staticmethod
    def backward(ctx, grad_out):
        g_final, u0, p0 = ctx.saved_tensors
        gf = g_final * grad_out
        w = 2.0 * ctx.lam * grad_out         # every slot adds lambda |row|^2 for its user row and for its positive's row
        return gf[:ctx.B], gf[ctx.B:], None, w * u0, w * p0, None


def full_softmax_loss(users_emb_final: Tensor, items_emb_final: Tensor, pos: Tensor, users_emb_0: Tensor,
                      pos_items_emb_0: Tensor, lambda_val: float) -> Tensor:
    """The exact softmax over the whole catalogue, the objective in_batch_softmax_loss and the sampled softmax of
    ranking_loss estimate: slot b's candidates are all rows of items_emb_final [I, D] with the logit <u_b, item_i>, no
    mask and no logq; pos [B] (int64) names each slot's positive.  users_emb_final and users_emb_0 are gathered blocks
    [B, D], pos_items_emb_0 [B, D] the positives' layer-0 rows (slots with equal ids must carry equal rows).  Gradients go
    to users_emb_final, items_emb_final (dense: every item row), users_emb_0 and pos_items_emb_0."""
    B = int(users_emb_final.shape[0])
    if pos.numel() != B or users_emb_0.shape != users_emb_final.shape or pos_items_emb_0.shape != users_emb_final.shape:
        raise ValueError(f"pos [{B}] and layer-0 blocks of shape {tuple(users_emb_final.shape)} expected")
    if items_emb_final.dim() != 2 or items_emb_final.shape[1] != users_emb_final.shape[1] or items_emb_final.shape[0] < 1:
        raise ValueError(f"items_emb_final: [I, {users_emb_final.shape[1]}] with I >= 1 expected")
    return _FullSoftmaxFn.apply(users_emb_final, items_emb_final, pos.reshape(B), users_emb_0, pos_items_emb_0,
                                float(lambda_val))


# ----------------------------------------------------------------------------------------------
# evaluation: batched on device (reference: per-user Python loops on the CPU)
# ----------------------------------------------------------------------------------------------
def create_adj_dict(edge_index: Tensor, from_nodes: Optional[Tensor] = None) -> dict:
    """{user: tensor of that user's items, in edge order} (utils/metrics_lightgcn.py:48-61).
    One stable sort instead of one mask per user."""
    src, dst = edge_index[0], edge_index[1]
    order = t.argsort(src, stable=True)
    s_sorted, d_sorted = src[order], dst[order]
    users = t.unique(src) if from_nodes is None else from_nodes
    lo = t.searchsorted(s_sorted, users)
    hi = t.searchsorted(s_sorted, users, right=True)
    return {int(u): d_sorted[int(a):int(b)] for u, a, b in zip(users.tolist(), lo.tolist(), hi.tolist())}


def create_adj_list(edge_index: Tensor, from_nodes: Optional[Tensor] = None) -> List[Tensor]:
    users = edge_index[0].unique(sorted=True) if from_nodes is None else from_nodes
    d = create_adj_dict(edge_index, from_nodes=users)
    return [d[int(u)] for u in users.tolist()]


def _exclusion_csr(users: Tensor, exclude_edges: Optional[Tensor], num_items: int) -> Optional[ops.DeviceCSR]:
    """CSR with one row per position in `users` holding that user's excluded item ids."""
    if exclude_edges is None or exclude_edges.numel() == 0:
        return None
    eu, ei = exclude_edges[0], exclude_edges[1]
    pos = t.searchsorted(users, eu)
    pos_c = pos.clamp(max=users.numel() - 1)
    keep = users[pos_c] == eu
    return ops.coo_to_csr(pos_c[keep].contiguous(), ei[keep].contiguous(), users.numel(), num_items, want_perm=False)


def topk_for_users(user_embedding: Tensor, item_embedding: Tensor, users: Tensor, exclude_edges: Optional[Tensor],
                   k: int) -> Tensor:
    """ids [len(users), k] — make_predictions_for_user for a sorted batch of users at once."""
    excl = _exclusion_csr(users, exclude_edges, item_embedding.shape[0])
    return ops.topk_excl(users.contiguous(), user_embedding, item_embedding, k, excl)


def make_predictions_for_user(user_embeddings: Tensor, article_embeddings: Tensor, user_id: int,
                              positive_items_for_user: dict, num_recommendations: int) -> Tensor:
    """Single-user form with the reference's signature (utils/metrics_lightgcn.py:125-142)."""
    dev = article_embeddings.device
    users = t.tensor([user_id], dtype=t.int64, device=dev)
    ignore = positive_items_for_user.get(user_id)
    excl = None
    if ignore is not None and len(ignore):
        ig = t.as_tensor(ignore, dtype=t.int64, device=dev)
        excl = t.stack([t.full_like(ig, user_id), ig])
    out = topk_for_users(user_embeddings, article_embeddings, users, excl, num_recommendations)[0]
    return out[out >= 0]


def rank_metrics(r: Tensor, gt_len: Tensor, k: int) -> Tuple[float, float, float]:
    """recall, precision, ndcg @ k from the hit matrix r [n, k] and |GT| per row — the arithmetic of
    utils/metrics.py:6-57 on tensors (device or host)."""
    rf = r.to(t.float32)
    hits = rf.sum(dim=-1)
    recall = (hits / gt_len.to(t.float32)).mean().item()
    precision = (hits.mean() / k).item()
    disc = 1.0 / t.log2(t.arange(2, k + 2, device=r.device, dtype=t.float32))
    ideal = (t.arange(k, device=r.device)[None, :] < gt_len.clamp(max=k)[:, None]).to(t.float32)
    idcg = (ideal * disc).sum(dim=1)
    dcg = (rf * disc).sum(dim=1)
    idcg[idcg == 0.0] = 1.0
    ndcg = dcg / idcg
    ndcg[t.isnan(ndcg)] = 0.0
    return recall, precision, ndcg.mean().item()


def get_metrics_lightgcn(model, edge_index: Tensor, exclude_edge_indices: List[Tensor], k: int,
                         embeddings: Optional[Tuple[Tensor, Tensor]] = None) -> Tuple[float, float, float]:
    """recall / precision / ndcg @ k of the layer-0 embeddings on the users of `edge_index`,
    never recommending items in `exclude_edge_indices` (utils/metrics_lightgcn.py:79-122).
    embeddings = (users [U, D], items [I, D]) scores with those tables instead (the propagated predictor)."""
    if embeddings is not None:
        ue, ie = embeddings[0].detach(), embeddings[1].detach()
    else:
        ue = model.users_emb.weight.detach()
        ie = model.items_emb.weight.detach()
    dev = ie.device
    edge_index = edge_index.to(dev)
    n_items = ie.shape[0]
    users = edge_index[0].unique()
    excl = t.cat([e.to(dev) for e in exclude_edge_indices], dim=1) if len(exclude_edge_indices) else None
    top = topk_for_users(ue, ie, users, excl, k)
    # r[u, j] = top[u, j] is one of u's positives in this split
    pos_of = t.searchsorted(users, edge_index[0])
    truth_keys = t.unique(pos_of * n_items + edge_index[1])
    pred_keys = t.arange(users.numel(), device=dev)[:, None] * n_items + top
    r = t.isin(pred_keys, truth_keys) & (top >= 0)
    gt_len = t.bincount(pos_of, minlength=users.numel())
    return rank_metrics(r, gt_len, k)


# ----------------------------------------------------------------------------------------------
# full-catalogue ranks of the held-out items (ops.rank_of_items): MRR, mean rank, AUC, MAP@K and recall@K at any K
# ----------------------------------------------------------------------------------------------
def _rows_of_csr(csr: ops.DeviceCSR, rows: Tensor) -> ops.DeviceCSR:
    """The CSR whose row p is row rows[p] of `csr` (ops.rank_of_items wants one exclusion row per query row, and a
    user's pairs share the user's row)."""
    ptr = csr.rowptr.to(t.int64)
    lens = (ptr[1:] - ptr[:-1])[rows]
    new_ptr = t.zeros(rows.numel() + 1, dtype=t.int64, device=rows.device)
    new_ptr[1:] = lens.cumsum(0)
    total = int(new_ptr[-1])
    if total >= 2 ** 31:
        raise ValueError("exclusion lists of the pairs exceed int32 indexing: rank the edges in several calls")
    src = t.repeat_interleave(ptr[:-1][rows] - new_ptr[:-1], lens) + t.arange(total, device=rows.device)
    return ops.DeviceCSR(rows.numel(), csr.n_cols, new_ptr.to(t.int32), csr.col[src].contiguous())


def ranks_for_edges(user_embedding: Tensor, item_embedding: Tensor, edge_index: Tensor,
                    exclude_edges: Optional[Tensor]) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """(users, pos_of, items, ranks, n_excluded) over the DISTINCT (user, item) pairs of `edge_index`, sorted by user (then
    item): users = the sorted distinct users, pos_of[p] = the position of pair p's user in `users`, items[p] its item,
    ranks[p] (int32) = how many items that `exclude_edges` does not list for the user score above it in top-K's order
    (-1: the pair itself is listed), n_excluded[p] (int32) = the user's distinct excluded items."""
    dev = item_embedding.device
    edge_index = edge_index.to(dev)
    n_items = item_embedding.shape[0]
    users = edge_index[0].unique()
    keys = t.unique(t.searchsorted(users, edge_index[0]) * n_items + edge_index[1])
    pos_of, items = keys // n_items, keys % n_items
    excl = _exclusion_csr(users, exclude_edges, n_items)
    if excl is not None:
        excl = _rows_of_csr(excl, pos_of)
    ranks, n_excluded = ops.rank_of_items(users[pos_of].contiguous(), items.contiguous(), user_embedding, item_embedding,
                                          excl, want_n_excluded=True)
    return users, pos_of, items, ranks, n_excluded


def full_rank_metrics(pos_of: Tensor, ranks: Tensor, n_items: int, n_excluded: Tensor, gt_len: Tensor, ks=(12,),
                      filtered: bool = False) -> dict:
    """Ranking metrics from one exact integer per held-out pair; pure torch (device or host), floats in float64.
    pos_of / ranks / n_excluded: per pair, as ranks_for_edges returns them (a user's pairs are DISTINCT items, so their
    ranks differ).  gt_len [n_users]: |GT| per user by get_metrics_lightgcn's rule, bincount over the split's edges, which
    counts a repeated edge every time it occurs.  Pairs with rank -1 are left out of everything ("excluded_pairs" says how
    many); m_u below is the number of a user's pairs that are left.
      recall@K, precision@K, ndcg@K   for any K <= n_items, over every user of gt_len: rank_metrics on the hit matrix of
                                      a top-K list (equal to it wherever K <= 1024 lets one be made)
      hits@K                          int64 [n_users]: the user's pairs with rank < K
      map@K                           per user 1 / min(K, m_u) * sum over pairs with rank < K of h / (rank + 1), h the
                                      1-based position of the pair among the user's own pairs by rank; mean over the users
                                      with m_u > 0
      mrr                             mean over those users of 1 / (best rank + 1)
      mean_rank                       mean over pairs of the rank (0-based)
      auc                             mean over pairs of 1 - r_f / (n_items - n_excluded - m_u), r_f the filtered rank; pairs
                                      whose denominator is 0 are left out (nan when none is left)
      filtered_rank                   int64 per pair (-1: left out): r_f = rank - (h - 1), the pair's rank against the
                                      items that are not the user's own positives
    filtered=True: every metric above takes r_f in the place of rank (h stays the position by rank).  Integer
    post-processing of the same ranks: nothing is scored again."""
    dev = ranks.device
    n_users = int(gt_len.numel())
    pos_of = pos_of.to(t.int64)
    rk = ranks.to(t.int64)
    valid = rk >= 0
    vp, vr = pos_of[valid], rk[valid]
    n_valid = int(vp.numel())
    m_u = t.bincount(vp, minlength=n_users)
    # position of every pair among its user's pairs by rank
    order = t.argsort(vp * (int(n_items) + 1) + vr)
    start = t.cumsum(m_u, 0) - m_u
    h0_sorted = t.arange(n_valid, device=dev) - start[vp[order]]
    h0 = t.empty_like(h0_sorted)
    h0[order] = h0_sorted
    r_f = vr - h0
    use = r_f if filtered else vr
    out = {"excluded_pairs": int((~valid).sum()), "pairs": n_valid}
    fr = t.full_like(rk, -1)
    fr[valid] = r_f
    out["filtered_rank"] = fr
    gt = gt_len.to(t.float64)
    has = m_u > 0
    n_has = max(int(has.sum()), 1)
    for k in ks:
        k = int(k)
        if not 1 <= k <= max(int(n_items), 1):
            raise ValueError(f"K must be in [1, n_items], got {k}")
        inside = use < k
        hits = t.bincount(vp[inside], minlength=n_users)
        out[f"hits@{k}"] = hits
        out[f"recall@{k}"] = float((hits.to(t.float64) / gt).mean()) if n_users else float("nan")
        out[f"precision@{k}"] = float(hits.to(t.float64).mean() / k) if n_users else float("nan")
        disc = 1.0 / t.log2(t.arange(2, k + 2, device=dev, dtype=t.float64))
        cum = t.cat([t.zeros(1, dtype=t.float64, device=dev), disc.cumsum(0)])
        idcg = cum[gt_len.to(t.int64).clamp(min=0, max=k)]
        idcg = t.where(idcg == 0.0, t.ones_like(idcg), idcg)
        dcg = t.zeros(n_users, dtype=t.float64, device=dev).index_add_(0, vp[inside], disc[use[inside]])
        out[f"ndcg@{k}"] = float((dcg / idcg).mean()) if n_users else float("nan")
        ap = t.zeros(n_users, dtype=t.float64, device=dev).index_add_(
            0, vp[inside], (h0[inside] + 1).to(t.float64) / (use[inside] + 1).to(t.float64))
        ap = ap / m_u.clamp(min=1, max=k).to(t.float64)
        out[f"map@{k}"] = float(ap[has].sum() / n_has) if n_valid else float("nan")
    best = t.full((n_users,), int(n_items), dtype=t.int64, device=dev).scatter_reduce_(0, vp, use, reduce="amin")
    out["mrr"] = float((1.0 / (best[has] + 1).to(t.float64)).sum() / n_has) if n_valid else float("nan")
    out["mean_rank"] = float(use.to(t.float64).mean()) if n_valid else float("nan")
    den = int(n_items) - n_excluded.to(t.int64)[valid] - m_u[vp]
    ok = den > 0
    out["auc"] = float((1.0 - r_f[ok].to(t.float64) / den[ok].to(t.float64)).mean()) if int(ok.sum()) else float("nan")
    return out


def get_full_rank_metrics_lightgcn(model, edge_index: Tensor, exclude_edge_indices: List[Tensor], ks=(12,),
                                   embeddings: Optional[Tuple[Tensor, Tensor]] = None, filtered: bool = False) -> dict:
    """full_rank_metrics of the layer-0 embeddings (or of `embeddings` = (users, items)) on the distinct pairs of
    `edge_index`, never ranking against items in `exclude_edge_indices`: the counterpart of get_metrics_lightgcn with the
    whole catalogue in view instead of the first k places.  Its recall / precision / ndcg @ K are get_metrics_lightgcn's."""
    if embeddings is not None:
        ue, ie = embeddings[0].detach(), embeddings[1].detach()
    else:
        ue = model.users_emb.weight.detach()
        ie = model.items_emb.weight.detach()
    dev = ie.device
    edge_index = edge_index.to(dev)
    excl = t.cat([e.to(dev) for e in exclude_edge_indices], dim=1) if len(exclude_edge_indices) else None
    users, pos_of, _, ranks, n_excluded = ranks_for_edges(ue, ie, edge_index, excl)
    gt_len = t.bincount(t.searchsorted(users, edge_index[0]), minlength=users.numel())
    return full_rank_metrics(pos_of, ranks, ie.shape[0], n_excluded, gt_len, ks=ks, filtered=filtered)
