"""CPU mirror of the recent-items recommender's rule of include/laplace_hip.h ("N5 recent-items recommender": mi_recent_items,
mi_pool_recent_f32, mi_topk_merge_max_f32 and pinsage.evaluation.RecentItemsRecommender on top of them), step for step in
numpy float32.  Scores of a query against the catalogue are the oracle's k-ordered fma chain (oracle.lightgcn_ref.scores_fma:
the arithmetic of the HIP top-K).  Test infrastructure only; the product never imports it."""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np
import torch as t

from oracle import lightgcn_ref as R

WINDOW = 64
NEG_INF = np.float32(-np.inf)


def weights(decay: float, n: int) -> np.ndarray:
    """w[r] = (float)pow((double)decay, r)."""
    return np.array([float(decay) ** r for r in range(n)], dtype=np.float64).astype(np.float32)


def history(row: Sequence[int], n_recent: int) -> List[int]:
    """The slots of one user: the window's entries most recent first, an entry dropped when a more recent position holds its
    item, the first n_recent survivors."""
    window = list(row)[-WINDOW:][::-1]           # position p = 0 is the last entry
    kept = [item for p, item in enumerate(window) if item not in window[:p]]
    return kept[:n_recent]


def recent_items(rows: Sequence[Sequence[int]], n_recent: int) -> Tuple[np.ndarray, np.ndarray]:
    """(items int64 [n_recent, n_users], n_slots int32 [n_users]); unused slots hold the slot-0 item."""
    n_users = len(rows)
    items = np.empty((n_recent, n_users), dtype=np.int64)
    n_slots = np.empty(n_users, dtype=np.int32)
    for u, row in enumerate(rows):
        if len(row) == 0:
            raise ValueError("every user needs at least one interaction")
        slots = history(row, n_recent)
        n_slots[u] = len(slots)
        items[:, u] = slots[0]
        items[:len(slots), u] = slots
    return items, n_slots


def pool_mean(items: np.ndarray, n_slots: np.ndarray, w: np.ndarray, h: np.ndarray) -> np.ndarray:
    """q[u] = acc / W with acc = acc + w[r] * h[item_r], W = W + w[r], r ascending: every operation one float32 rounding."""
    h = np.asarray(h, dtype=np.float32)
    w = np.asarray(w, dtype=np.float32)
    n_users = items.shape[1]
    q = np.empty((n_users, h.shape[1]), dtype=np.float32)
    for u in range(n_users):
        acc = np.zeros(h.shape[1], dtype=np.float32)
        W = np.float32(0.0)
        for r in range(int(n_slots[u])):
            p = (w[r] * h[items[r, u]]).astype(np.float32)
            acc = (acc + p).astype(np.float32)
            W = np.float32(W + w[r])
        q[u] = (acc / W).astype(np.float32)
    return q


def topk_excl(scores: np.ndarray, rows: Sequence[Sequence[int]], K: int) -> Tuple[np.ndarray, np.ndarray]:
    """ops.topk_excl on given scores [n_q, n_items]: per row the K best ids by (score desc, id asc) outside rows[q]; -1 / -inf
    pads."""
    n_q, n_items = scores.shape
    ids = np.full((n_q, K), -1, dtype=np.int64)
    sc = np.full((n_q, K), NEG_INF, dtype=np.float32)
    for q in range(n_q):
        mask = np.ones(n_items, dtype=bool)
        mask[np.asarray(rows[q], dtype=np.int64)] = False
        cand = np.flatnonzero(mask)
        order = cand[np.lexsort((cand, -scores[q, cand].astype(np.float64)))][:K]
        ids[q, :order.size] = order
        sc[q, :order.size] = scores[q, order]
    return ids, sc


def merge_max(ids: np.ndarray, scores: np.ndarray, n_slots: np.ndarray, w: np.ndarray, k_out: int) -> Tuple[np.ndarray, np.ndarray]:
    """mi_topk_merge_max_f32: ids / scores [n_lists, n_q, k_in].  The candidates of query q are the entries of lists
    r < n_slots[q] with id != -1; an item's score is the maximum of float32(w[r] * score) + 0 over its entries; the k_out best
    by (score desc, id asc), -1 / -inf pads."""
    n_lists, n_q, k_in = ids.shape
    w = np.asarray(w, dtype=np.float32)
    out_ids = np.full((n_q, k_out), -1, dtype=np.int64)
    out_sc = np.full((n_q, k_out), NEG_INF, dtype=np.float32)
    weighted = (w[:, None, None] * np.asarray(scores, dtype=np.float32)).astype(np.float32) + np.float32(0.0)
    best = np.empty(max(int(ids.max()) + 1, 1), dtype=np.float32)
    for q in range(n_q):
        ns = max(0, min(int(n_slots[q]), n_lists))
        i, s = ids[:ns, q].ravel(), weighted[:ns, q].ravel()
        i, s = i[i >= 0], s[i >= 0]
        best[:] = NEG_INF
        np.maximum.at(best, i, s)                 # an item's score: the maximum over its entries
        cand = np.unique(i)
        order = cand[np.lexsort((cand, -best[cand].astype(np.float64)))][:k_out]
        out_ids[q, :order.size] = order
        out_sc[q, :order.size] = best[order]
    return out_ids, out_sc


def scores_fma(queries: np.ndarray, h: np.ndarray) -> np.ndarray:
    return R.scores_fma(t.from_numpy(np.ascontiguousarray(queries, dtype=np.float32)),
                        t.from_numpy(np.ascontiguousarray(h, dtype=np.float32))).numpy()


def recommend(rows: Sequence[Sequence[int]], h: np.ndarray, n_recent: int, pool: str, decay: float, K: int):
    """RecentItemsRecommender(n_recent, pool, decay).recommend(rows, K, None, h, want_scores=True)."""
    h = np.asarray(h, dtype=np.float32)
    items, n_slots = recent_items(rows, n_recent)
    w = weights(decay, n_recent)
    if pool == "mean":
        return topk_excl(scores_fma(pool_mean(items, n_slots, w, h), h), rows, K)
    uniq, at = np.unique(items, return_inverse=True)     # every slot's query is a catalogue row: score each once
    at = at.reshape(items.shape)
    row_scores = scores_fma(h[uniq], h)
    lists = [topk_excl(row_scores[at[r]], rows, K) for r in range(n_recent)]
    return merge_max(np.stack([l[0] for l in lists]), np.stack([l[1] for l in lists]), n_slots, w, K)


def brute_force_max(rows: Sequence[Sequence[int]], h: np.ndarray, n_recent: int, K: int) -> Tuple[np.ndarray, np.ndarray]:
    """decay = 1 by its closed form: the top-K of max_r h[item_r] . h[i] over the items outside the user's row (`h` must make
    every dot product exact: the + 0 of the rule then only removes the sign of a zero, as here)."""
    h = np.asarray(h, dtype=np.float32)
    full = (h.astype(np.float64) @ h.astype(np.float64).T)
    assert np.array_equal(full, full.astype(np.float32).astype(np.float64)), "h does not make the dot products exact"
    score = np.stack([full[history(row, n_recent)].max(axis=0) for row in rows]).astype(np.float32) + np.float32(0.0)
    return topk_excl(score, rows, K)


# ---- shared test data -----------------------------------------------------------------------------------------------------
def dyadic_table(n_items: int, d: int = 16, seed: int = 0) -> np.ndarray:
    """float32 [n_items, d] of multiples of 1/4 in [-2, 2] without an all-zero row: every product is a multiple of 1/16 and
    every partial sum stays below 2^7, so a dot product is exact in float32 in any order (and times a power of two)."""
    rng = np.random.default_rng(seed)
    h = rng.integers(-8, 9, (n_items, d)).astype(np.float32) / np.float32(4.0)
    zero = ~h.any(axis=1)
    h[zero, 0] = 0.25
    return h


def history_rows(n_items: int, n_recent: int, seed: int = 0, n_random: int = 30) -> List[List[int]]:
    """Rows that walk the history rule's edges: lengths 1, n_recent, 63, 64, 65 and 300 with repeats, one item repeated, all
    distinct, a (MAX + 1)-th distinct item just outside the window, distinct items that only exist before the window, and
    n_random ordinary rows."""
    rng = np.random.default_rng(seed)
    pool = lambda n, k: rng.choice(n_items, size=k, replace=False)
    rows: List[List[int]] = []
    for n in (1, n_recent, 63, 64, 65, 300):
        rows.append(pool(n_items, min(40, n_items))[rng.integers(0, min(40, n_items), n)].tolist())      # repeats
    rows.append([int(rng.integers(0, n_items))] * 70)                                                    # one item repeated
    rows.append(pool(n_items, 65).tolist())                                                              # 65 distinct
    p = pool(n_items, 17)
    rows.append([int(p[16])] * 3 + [int(p[16 - 1 - (j % 16)]) for j in range(64)])   # 16 distinct in the window, a 17th before it
    p = pool(n_items, 12)
    rows.append(p[5:].tolist() * 2 + p[:5][rng.integers(0, 5, 64)].tolist())         # at most 5 distinct in the window, 7 more before
    rows.append([int(p[0]), int(p[1]), int(p[0])])                                   # the latest item again further back
    for _ in range(n_random):
        n = int(rng.integers(1, 25))
        rows.append(rng.integers(0, n_items, n).tolist())
    return rows


def csr_of(rows: Sequence[Sequence[int]]) -> Tuple[np.ndarray, np.ndarray]:
    """(ptr int32 [n + 1], idx int32 [nnz]) of the rows in their order."""
    ptr = np.zeros(len(rows) + 1, dtype=np.int32)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    idx = np.array([i for r in rows for i in r], dtype=np.int32)
    return ptr, idx
