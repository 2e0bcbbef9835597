"""CPU mirror of the random-walk matcher's rule of include/laplace_hip.h ("N3c random-walk matcher": mi_match_random_walks_i32,
data.matching.RandomWalkMatcher, pinsage.evaluation.RandomWalkRecommender), draw for draw in numpy: the Philox counters of
oracle.philox in the PinSAGE layout (oracle.pinsage_ref._words), the hop of oracle.pinsage_ref._hop, the history of
tests/recent_items_emulation.history, float32 arithmetic with one rounding per operation.  Test infrastructure only; the
product never imports it."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from oracle import pinsage_ref as PR
from oracle.philox import philox4x32

from recent_items_emulation import history

P_MATCH_WALK = 17
MAX_VISITS = 4096
# the correctly rounded float32 root of every possible count: float64 sqrt is correctly rounded and 53 >= 2 * 24 + 2 bits make
# the second rounding innocuous
ROOTS = np.sqrt(np.arange(MAX_VISITS + 1, dtype=np.float64)).astype(np.float32)


@dataclass(frozen=True)
class Rule:
    num_walks: int
    walk_length: int
    restart_prob: float
    n_recent: int
    boost: str
    exclude_seen: bool


def _walk_words(n: int, u: int, seed: int, step: int):
    """The draws pw(17, a, 0, u, seed, step) for a = 0 .. n - 1 in one vectorised Philox call: three uint32 lists."""
    c3 = (P_MATCH_WALK & 0xFF) | ((step & 0xFFFFFF) << 8)
    k0, k1 = seed & 0xFFFFFFFF, ((seed >> 32) ^ (step >> 24)) & 0xFFFFFFFF
    w = philox4x32(np.arange(n, dtype=np.uint64), 0, u & 0xFFFFFFFF, c3, k0, k1)
    return w[0].tolist(), w[1].tolist(), w[2].tolist()


def assert_layout_is_the_oracles(seed: int = 0x1234567890ABCDEF, step: int = 0x3456789) -> None:
    """_walk_words is oracle.pinsage_ref._words, vectorised: checked once by the CPU tests."""
    w0, w1, w2 = _walk_words(5, 77, seed, step)
    for a in range(5):
        assert PR._words(P_MATCH_WALK, a, 0, 77, seed, step)[:3] == [w0[a], w1[a], w2[a]]


def slot_counts(u: int, item_users: PR.Csr, user_items: PR.Csr, rule: Rule, seed: int, step: int) -> List[Dict[int, int]]:
    """c[r][i] of user u: one dict of visit counts per slot (an empty list for an empty row)."""
    slots = history([int(i) for i in user_items[u]], rule.n_recent)
    R = len(slots)
    counts: List[Dict[int, int]] = [{} for _ in range(R)]
    if R == 0:
        return counts
    W, L = rule.num_walks, rule.walk_length
    thr = int(rule.restart_prob * 4294967296.0)
    w0, w1, w2 = _walk_words(W * L, u, seed, step)
    for w in range(W):
        r = w % R
        cur = slots[r]
        for tr in range(L):
            a = w * L + tr
            if tr > 0 and w2[a] < thr:
                break
            cur = PR._hop(cur, item_users, user_items, w0[a], w1[a])
            if cur == -1:
                break
            counts[r][cur] = counts[r].get(cur, 0) + 1
    return counts


def scores(counts: List[Dict[int, int]], boost: str) -> Dict[int, np.float32]:
    """s(i) of every visited item: 'sum' the total count, 'multi_hit' (sum_r sqrt(c[r][i]))^2 in float32, r ascending from 0."""
    out: Dict[int, np.float32] = {}
    for i in sorted(set().union(*counts)) if counts else []:
        if boost == "sum":
            out[i] = np.float32(sum(c.get(i, 0) for c in counts))
        else:
            acc = np.float32(0.0)
            for c in counts:
                if c.get(i, 0) > 0:
                    acc = np.float32(acc + ROOTS[c[i]])
            out[i] = np.float32(acc * acc)
    return out


def match_user(u: int, item_users: PR.Csr, user_items: PR.Csr, rule: Rule, k: int, seed: int, step: int = 0, counts=None):
    """(ids int32 [k] with -1 pads, scores float32 [k] with 0 pads, count) of one user.  counts: slot_counts(u, ...) when the
    caller has them already (they do not depend on boost, exclude_seen or k)."""
    if rule.num_walks * rule.walk_length > MAX_VISITS:
        raise ValueError("num_walks * walk_length is above 4096")
    s = scores(slot_counts(u, item_users, user_items, rule, seed, step) if counts is None else counts, rule.boost)
    if rule.exclude_seen:
        seen = set(int(i) for i in user_items[u])
        s = {i: v for i, v in s.items() if i not in seen}
    order = sorted(s, key=lambda i: (-float(s[i]), i))
    ids = np.full(k, -1, dtype=np.int32)
    sc = np.zeros(k, dtype=np.float32)
    top = order[:k]
    ids[:len(top)] = top
    sc[:len(top)] = [s[i] for i in top]
    return ids, sc, len(order)


def match(users: Sequence[int], item_users: PR.Csr, user_items: PR.Csr, rule: Rule, k: int, seed: int, step: int = 0,
          cache: Optional[dict] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """mi_match_random_walks_i32 for the listed users: (ids int32 [n, k], scores float32 [n, k], counts int32 [n]).  A user's row
    depends on the user alone: `cache` (user -> row) lets callers share rows between query lists."""
    cache = {} if cache is None else cache
    ids = np.empty((len(users), k), dtype=np.int32)
    sc = np.empty((len(users), k), dtype=np.float32)
    cnt = np.empty(len(users), dtype=np.int32)
    for row, u in enumerate(users):
        u = int(u)
        if u not in cache:
            cache[u] = match_user(u, item_users, user_items, rule, k, seed, step)
        ids[row], sc[row], cnt[row] = cache[u]
    return ids, sc, cnt


# ---- shared test data -----------------------------------------------------------------------------------------------------
EMPTY_USERS, UNSOLD = (0, 7, 299), 33
LONE_USER, LONE_ITEM = 300, 90        # the user's only item, which nobody else holds: with exclude_seen no proposal
DUP_USER = 301                        # 150 entries over 10 items: more than the 64-entry window, many duplicates
LONG_USER = 302                       # ~3 000 entries over 60 items: the exclusion search's long row
N_USERS, N_ITEMS = 303, 91


def small_graph(seed: int = 0):
    """(u, a) edge arrays in transaction order: a shuffled log of 300 users x 90 items x 2 500 distinct entries and 100 repeats
    (the recipe of tests/test_gpu_cooccurrence._small_graph), three users without entries, one unsold item, and the three
    users above.  AdjList.from_edges is stable, so both adjacency lists keep this order."""
    g = np.random.default_rng(seed)
    U, A = 300, 90
    ok = np.array([k for k in range(U * A) if k % A != UNSOLD and k // A not in EMPTY_USERS])
    keys = g.choice(ok, size=2500, replace=False)
    keys = np.concatenate([keys, g.choice(keys, size=100, replace=True)])
    u, a = keys // A, keys % A
    sold = np.setdiff1d(np.arange(A), [UNSOLD])
    dup_items, long_items = g.choice(sold, size=10, replace=False), g.choice(sold, size=60, replace=False)
    u = np.concatenate([u, [LONE_USER], np.full(150, DUP_USER), np.full(3000, LONG_USER)])
    a = np.concatenate([a, [LONE_ITEM], dup_items[g.integers(0, 10, 150)], long_items[g.integers(0, 60, 3000)]])
    p = g.permutation(u.size)
    return u[p].astype(np.int64), a[p].astype(np.int64)


def csr_pair(u: np.ndarray, a: np.ndarray, n_users: int, n_items: int) -> Tuple[PR.Csr, PR.Csr]:
    """(item_users, user_items) of an edge log, both in log order (what AdjList.from_edges builds)."""
    def one(src, dst, n):
        order = np.argsort(src, kind="stable")
        ptr = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(np.bincount(src, minlength=n), out=ptr[1:])
        return PR.Csr(ptr, dst[order])
    return one(a, u, n_items), one(u, a, n_users)
