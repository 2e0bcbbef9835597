"""The reference of the full-rank tests: the rule of include/laplace_hip.h (K10r) in numpy on the oracle's fma-chain scores, and
the metrics of utils.metrics_lightgcn.full_rank_metrics in float64 with plain per-user Python loops.  Nothing here is shared
with the code under test."""
import math

import numpy as np


def score_key(s):
    """score_key of csrc/score_panel.hpp on a float32 array: -0 -> +0, then the monotone map to uint32."""
    u = (np.asarray(s, dtype=np.float32) + np.float32(0.0)).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))


def ranks(scores, target, excl):
    """(rank int32 [n_q], score float32 [n_q], n_excluded int32 [n_q]).  scores: the oracle's [n_q, n_items] float32 (row p is
    user uid[p]); target: int64 [n_q]; excl: a list of id arrays per row (unsorted, repeats, out-of-range ids allowed) or None."""
    scores = np.asarray(scores, dtype=np.float32)
    n_q, n_items = scores.shape
    rank = np.full(n_q, -1, dtype=np.int32)
    score = np.zeros(n_q, dtype=np.float32)
    n_ex = np.zeros(n_q, dtype=np.int32)
    ids = np.arange(n_items)
    for p in range(n_q):
        gone = np.zeros(n_items, dtype=bool)
        if excl is not None and len(excl[p]):
            e = np.asarray(excl[p], dtype=np.int64)
            gone[e[(e >= 0) & (e < n_items)]] = True
        n_ex[p] = int(gone.sum())
        t = int(target[p])
        if not 0 <= t < n_items:
            continue
        score[p] = scores[p, t]
        if gone[t]:
            continue
        key = score_key(scores[p])
        beats = (key > key[t]) | ((key == key[t]) & (ids < t))
        rank[p] = int((beats & ~gone & (ids != t)).sum())
    return rank, score, n_ex


def metrics(pos_of, rank, n_items, n_excluded, gt_len, ks, filtered=False):
    """The dict of full_rank_metrics, by loops over users and pairs in Python floats (float64)."""
    n_users = len(gt_len)
    pairs = [[] for _ in range(n_users)]                    # per user: (rank, pair index) of the pairs that are left
    for p, (u, r) in enumerate(zip(pos_of, rank)):
        if r >= 0:
            pairs[int(u)].append((int(r), p))
    out = {"excluded_pairs": int(sum(1 for r in rank if r < 0)), "pairs": int(sum(len(x) for x in pairs))}
    fr = [-1] * len(rank)
    h_of, use_of = {}, {}
    for u in range(n_users):
        pairs[u].sort()
        for h0, (r, p) in enumerate(pairs[u]):
            fr[p] = r - h0
            h_of[p] = h0 + 1
            use_of[p] = fr[p] if filtered else r
    out["filtered_rank"] = fr
    with_pairs = [u for u in range(n_users) if pairs[u]]
    for k in ks:
        hits, rec, ndcg, ap = [], [], [], []
        for u in range(n_users):
            inside = [p for _, p in pairs[u] if use_of[p] < k]
            hits.append(len(inside))
            rec.append(len(inside) / float(gt_len[u]))
            dcg = sum(1.0 / math.log2(use_of[p] + 2) for p in inside)
            idcg = sum(1.0 / math.log2(j + 2) for j in range(min(int(gt_len[u]), k)))
            ndcg.append(dcg / (idcg if idcg != 0.0 else 1.0))
            if pairs[u]:
                ap.append(sum(h_of[p] / (use_of[p] + 1.0) for p in inside) / min(k, len(pairs[u])))
        out[f"hits@{k}"] = hits
        out[f"recall@{k}"] = sum(rec) / n_users
        out[f"precision@{k}"] = sum(hits) / n_users / k
        out[f"ndcg@{k}"] = sum(ndcg) / n_users
        out[f"map@{k}"] = sum(ap) / len(ap) if ap else float("nan")
    if with_pairs:
        out["mrr"] = sum(1.0 / (min(use_of[p] for _, p in pairs[u]) + 1.0) for u in with_pairs) / len(with_pairs)
        out["mean_rank"] = sum(use_of.values()) / len(use_of)
    else:
        out["mrr"] = out["mean_rank"] = float("nan")
    auc = []
    for u in with_pairs:
        for _, p in pairs[u]:
            den = n_items - int(n_excluded[p]) - len(pairs[u])
            if den > 0:
                auc.append(1.0 - fr[p] / den)
    out["auc"] = sum(auc) / len(auc) if auc else float("nan")
    return out
