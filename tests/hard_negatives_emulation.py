"""CPU mirror of the hard-negative rule of include/laplace_hip.h (mi_pinsage_hard_negatives), draw for draw in numpy:
the same Philox counters, the same walk law as oracle.pinsage_ref.pinsage_neighbors, the same (count desc, id asc) ranking.
Test infrastructure only; the product never imports it."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Tuple

import numpy as np

from oracle import pinsage_ref as PR
from oracle.philox import philox4x32

P_HARD_PICK, P_HARD_WALK = 15, 16


@dataclass(frozen=True)
class Rule:
    num_walks: int
    walk_length: int
    restart_prob: float
    rank_lo: int
    rank_hi: int
    share: float


def _walk_words(n: int, h: int, seed: int, step: int):
    """The draws pw(16, a, 0, h, seed, step) for a = 0 .. n - 1 in one vectorised Philox call: three uint32 lists."""
    c3 = (P_HARD_WALK & 0xFF) | ((step & 0xFFFFFF) << 8)
    k0, k1 = seed & 0xFFFFFFFF, ((seed >> 32) ^ (step >> 24)) & 0xFFFFFFFF
    w = philox4x32(np.arange(n, dtype=np.uint64), 0, h & 0xFFFFFFFF, c3, k0, k1)
    return w[0].tolist(), w[1].tolist(), w[2].tolist()


def walk_counts(h: int, item_users: PR.Csr, user_items: PR.Csr, rule: Rule, seed: int, step: int) -> Dict[int, int]:
    """Visit counts of the rule's walks from head h (h itself and the pair's tail still in)."""
    W, L = rule.num_walks, rule.walk_length
    thr = int(rule.restart_prob * 4294967296.0)
    w0, w1, w2 = _walk_words(W * L, h, seed, step)
    counts: Dict[int, int] = {}
    for wk in range(W):
        cur = h
        for tr in range(L):
            k = wk * L + tr
            if tr > 0 and w2[k] < thr:
                break
            cur = PR._hop(cur, item_users, user_items, w0[k], w1[k])
            if cur == -1:
                break
            counts[cur] = counts.get(cur, 0) + 1
    return counts


def ranked(counts: Dict[int, int], h: int, tl: int) -> List[Tuple[int, int]]:
    """[(item, count)] by (count desc, id asc) with the head and the tail removed."""
    return sorted(((v, c) for v, c in counts.items() if v != h and v != tl), key=lambda vc: (-vc[1], vc[0]))


def selected(b: int, share: float, seed: int, step: int) -> Tuple[bool, int]:
    """(pair b is hard, the pick word pk.c[1])."""
    pk = PR._words(P_HARD_PICK, b, 0, 0, seed, step)
    return (share >= 1.0 or pk[0] < int(share * 4294967296.0)), pk[1]


def hard_item_pairs(batch: int, n_items: int, item_users: PR.Csr, user_items: PR.Csr, rule: Rule, seed: int, step: int):
    """All `batch` pairs of (seed, step), dead ones included (tail -1): heads, tails, negatives after the rule, the rank
    taken per pair (-1: uniform negative kept or dead pair) and per pair a word saying what happened:
    'dead', 'uniform' (not selected), 'fallback' (window empty), 'truncated' (m < rank_hi) or 'full'.
    Pair b does not depend on `batch`: a smaller batch is a prefix."""
    heads = np.empty(batch, dtype=np.int64)
    tails = np.empty(batch, dtype=np.int64)
    negs = np.empty(batch, dtype=np.int64)
    ranks = np.full(batch, -1, dtype=np.int32)
    what: List[str] = []
    cache: Dict[int, Dict[int, int]] = {}
    for b in range(batch):
        w = PR._words(PR.P_HEAD, b, 0, 0, seed, step)
        h = w[0] % n_items
        tl = PR._hop(h, item_users, user_items, w[1], w[2])
        heads[b], tails[b] = h, tl
        negs[b] = PR._words(PR.P_NEG, b, 0, 0, seed, step)[0] % n_items
        if tl == -1:
            what.append("dead")
            continue
        hard, pick = selected(b, rule.share, seed, step)
        if not hard:
            what.append("uniform")
            continue
        if h not in cache:
            cache[h] = walk_counts(h, item_users, user_items, rule, seed, step)
        order = ranked(cache[h], h, tl)
        m = len(order)
        end = min(rule.rank_hi, m)
        if end <= rule.rank_lo:
            what.append("fallback")
            continue
        r = rule.rank_lo + pick % (end - rule.rank_lo)
        negs[b], ranks[b] = order[r][0], r
        what.append("truncated" if m < rule.rank_hi else "full")
    return heads, tails, negs, ranks, what
