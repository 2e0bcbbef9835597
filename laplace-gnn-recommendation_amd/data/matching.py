"""Candidate matchers for evaluation (reference: data/matching/*.py, `Matcher.get_matches(user_id) ->
LongTensor`).  Same outputs, computed over the CSR adjacency instead of dicts of lists, and lazily:
the reference materialises every article of every co-purchasing user and then keeps the first k.

  LightGCNMatcher              first k of the user's LightGCN top-N row (data/matching/lightgcn.py:5-11);
                               fed directly by run_pipeline_lightgcn.save_predictions' [U, N] tensor
  PopularItemsMatcher          first k most popular items (data/matching/fashion/popular_items.py)
  UsersWithCommonItemsMatcher  first k entries of: for each article of the user (list order), for each
                               user of that article (list order, the user itself included), all their
                               articles (data/matching/users_with_common_purchases.py:14-26)

  UsersSameLocationMatcher     first k entries of: for each customer at the user's location (list order, the user
                               itself included), all their articles (data/matching/fashion/users_same_location.py:8-25;
                               commented out of the reference's get_matchers, kept here the same way)

  ItemCooccurrenceMatcher      NO reference counterpart — the scored form of the walk above: item-to-item co-purchase
                               similarity c(i, j) = (A^T A)[i, j] (raw, or cosine c / sqrt(d_i d_j)), the T best
                               neighbours kept per item; a user's candidates are the k best j by the sum of the neighbour
                               scores over the items the user holds (all, or the last n_recent), optionally without the
                               items the user already has.  Device: mi_cooc_items_topt + mi_match_cooc_i32
                               (csrc/cooccurrence.hip); the host get_matches restates the definitions in NumPy and is the
                               checker (tests/test_cooccurrence_cpu.py, tests/test_gpu_cooccurrence.py)

  RandomWalkMatcher            NO reference counterpart — Pixie-style candidates: walks of item -> user -> item traversals
                               from the user's last n_recent distinct items (PinSAGE's walk law and Philox draws, keyed on
                               the user id), visit counts per start slot, score = their sum or Pixie's multi-hit boost
                               (sum_r sqrt(c_r))^2, the k best by (score desc, id asc), optionally without the items the
                               user already has.  No training and no table: an edge counts the moment it is in the
                               adjacency.  Device only: mi_match_random_walks_i32 (csrc/walk_match.hip); the checker is the
                               numpy mirror tests/random_walk_matcher_emulation.py (tests/test_random_walk_matcher_cpu.py,
                               tests/test_gpu_random_walk_matcher.py)

The first four are pinned against the reference's own classes: tests/golden/matchers.pt (tests/make_golden.py runs them on
small dict-of-list files) — host forms in tests/test_oracle_golden.py, device forms in tests/test_gpu_matching.py.

Device forms: every matcher also answers for ALL users at once as a device tensor [U, k] (int64, -1 = no
proposal) through `matches_for_all_device(num_users, device)` — the common-purchase expansion is the HIP kernel
mi_match_common_items_i32, popularity is a device argsort of the degrees, the LightGCN rows are a slice of the top-K
dump that is already on the device — and `device_sampler.candidate_csr_device` turns them into the candidate CSR the
evaluation sampler reads, with no per-user host loop.  The host `get_matches` stays as the checker.
"""
from __future__ import annotations

from typing import List

import numpy as np
import torch as t
from torch import Tensor

from .dataset import AdjList


class Matcher:
    def get_matches(self, user_id: int) -> Tensor:
        raise NotImplementedError


class LightGCNMatcher(Matcher):
    def __init__(self, top_articles_per_user: Tensor, k: int):
        self._top_dev = top_articles_per_user if top_articles_per_user.is_cuda else None  # save_predictions' dump, kept where it is
        self.top, self.k = top_articles_per_user.cpu(), int(k)

    def get_matches(self, user_id: int) -> Tensor:
        row = self.top[user_id][: self.k]
        return row[row >= 0]

    def matches_for_all(self, num_users: int):
        """[num_users, k] proposals at once (-1 = none): what the device sampler's evaluation mode consumes."""
        return self.top[:num_users, : self.k].numpy()

    def matches_for_all_device(self, num_users: int, device) -> Tensor:
        src = self._top_dev if getattr(self, "_top_dev", None) is not None else self.top
        return src[:num_users, : self.k].to(device=device, dtype=t.int64)


class PopularItemsMatcher(Matcher):
    def __init__(self, popular_items, k: int):
        self.popular_items, self.k = t.as_tensor(popular_items).to(t.long), int(k)

    @classmethod
    def from_adjacency(cls, articles_adj, k: int) -> "PopularItemsMatcher":
        adj = AdjList(articles_adj) if not isinstance(articles_adj, AdjList) else articles_adj
        deg = np.diff(adj.ptr)
        order = np.argsort(-deg, kind="stable")
        return cls(order.copy(), k)

    def get_matches(self, user_id: int) -> Tensor:
        return self.popular_items[: self.k].cpu()

    def matches_for_all(self, num_users: int):
        return np.broadcast_to(self.popular_items[: self.k].cpu().numpy(), (num_users, min(self.k, self.popular_items.numel())))

    @classmethod
    def from_degrees_device(cls, article_degrees: Tensor, k: int) -> "PopularItemsMatcher":
        """Most popular first, ties by id (stable), computed where the degrees live."""
        return cls(t.argsort(article_degrees.to(t.int64), descending=True, stable=True), k)

    def matches_for_all_device(self, num_users: int, device) -> Tensor:
        row = self.popular_items[: self.k].to(device)
        return row[None, :].expand(num_users, row.numel())


class UsersWithCommonItemsMatcher(Matcher):
    def __init__(self, users_adj, articles_adj, k: int):
        self.users = users_adj if isinstance(users_adj, AdjList) else AdjList(users_adj)
        self.articles = articles_adj if isinstance(articles_adj, AdjList) else AdjList(articles_adj)
        self.k = int(k)

    def matches_for_all_device(self, num_users: int, device) -> Tensor:
        from .. import ops
        dev = t.device(device)
        if dev.type == "cuda" and dev.index is None:       # "cuda" and "cuda:0" are the same place: compare normalised devices
            dev = t.device("cuda", t.cuda.current_device())
        if num_users > len(self.users):
            raise IndexError(f"{num_users} query users but the purchase lists cover {len(self.users)}")
        if getattr(self, "_dev", None) is None or self._dev[0].device != dev:
            to32 = lambda a: t.from_numpy(np.ascontiguousarray(a.astype(np.int32))).to(dev)
            self._dev = (to32(self.users.ptr), to32(self.users.idx), to32(self.articles.ptr), to32(self.articles.idx))
        out, _ = ops.match_common_items(*self._dev, self.k, n_queries=num_users)
        return out.to(t.int64)

    def get_matches(self, user_id: int) -> Tensor:
        out: List[np.ndarray] = []
        have = 0
        for a in self.users[user_id]:
            for v in self.articles[int(a)]:
                lst = self.users[int(v)]
                out.append(lst)
                have += len(lst)
                if have >= self.k:
                    return t.from_numpy(np.concatenate(out)[: self.k].astype(np.int64))
        return t.from_numpy(np.concatenate(out).astype(np.int64)) if out else t.empty(0, dtype=t.long)


class UsersSameLocationMatcher(Matcher):
    def __init__(self, customers_per_location, location_for_user, users_adj, k: int):
        """customers_per_location: dict location -> [customer ids] (customers_per_location.pt); location_for_user: dict
        or array customer -> location (location_for_user.pt); users_adj: edges_<split>.pt."""
        self.users = users_adj if isinstance(users_adj, AdjList) else AdjList(users_adj)
        n_users = len(self.users)
        if isinstance(location_for_user, dict):
            loc = np.full(n_users, -1, dtype=np.int64)
            for u, l in location_for_user.items():
                if 0 <= int(u) < n_users:
                    loc[int(u)] = int(l)
        else:
            loc = np.asarray(location_for_user, dtype=np.int64)
        self.location_for_user = loc
        n_loc = max([int(loc.max()) + 1 if loc.size else 0] + [int(l) + 1 for l in customers_per_location])
        self.customers = AdjList({int(l): list(v) for l, v in customers_per_location.items()}, n_loc)
        self.k = int(k)
        # the device kernel indexes the customers' purchase lists and the location table with these ids unchecked: validate once
        idx = np.asarray(self.customers.idx)
        if idx.size and (int(idx.min()) < 0 or int(idx.max()) >= n_users):
            raise IndexError(f"customers_per_location names customer {int(idx.max())} but there are {n_users} customers")
        if loc.size and int(loc.max()) >= n_loc:
            raise IndexError("location_for_user names a location beyond customers_per_location")

    def get_matches(self, user_id: int) -> Tensor:
        loc = int(self.location_for_user[user_id])
        out: List[np.ndarray] = []
        have = 0
        if loc >= 0:
            for v in self.customers[loc]:
                lst = self.users[int(v)]
                out.append(lst)
                have += len(lst)
                if have >= self.k:
                    break
        return t.from_numpy(np.concatenate(out)[: self.k].astype(np.int64)) if out else t.empty(0, dtype=t.long)

    def matches_for_all_device(self, num_users: int, device) -> Tensor:
        from .. import ops
        dev = t.device(device)
        if dev.type == "cuda" and dev.index is None:       # "cuda" and "cuda:0" are the same place: compare normalised devices
            dev = t.device("cuda", t.cuda.current_device())
        if num_users > self.location_for_user.size:
            raise IndexError(f"{num_users} query users but location_for_user has {self.location_for_user.size} entries")
        if getattr(self, "_dev", None) is None or self._dev[0].device != dev:
            to32 = lambda a: t.from_numpy(np.ascontiguousarray(np.asarray(a).astype(np.int32))).to(dev)
            self._dev = (to32(self.location_for_user), to32(self.customers.ptr), to32(self.customers.idx),
                         to32(self.users.ptr), to32(self.users.idx))
        out, _ = ops.match_same_location(*self._dev, self.k, n_queries=num_users)
        return out.to(t.int64)


class ItemCooccurrenceMatcher(Matcher):
    """Scored item co-occurrence candidates (include/laplace_hip.h, N3b, states the contract).  Not in get_matchers: the
    reference has no such matcher, callers add it to their list themselves."""

    def __init__(self, users_adj, articles_adj, k: int, *, neighbors: int = 32, weighting: str = "cosine",
                 n_recent=None, exclude_seen: bool = False):
        self.users = users_adj if isinstance(users_adj, AdjList) else AdjList(users_adj)
        self.articles = articles_adj if isinstance(articles_adj, AdjList) else AdjList(articles_adj)
        if not 1 <= int(neighbors) <= 64:
            raise ValueError(f"neighbors must be within 1..64, got {neighbors}")
        if weighting not in ("count", "cosine"):
            raise ValueError(f"weighting must be 'count' or 'cosine', got {weighting!r}")
        if int(k) <= 0 or (n_recent is not None and int(n_recent) <= 0):
            raise ValueError("k and n_recent must be positive")
        self.k, self.neighbors, self.weighting = int(k), int(neighbors), weighting
        self.n_recent = None if n_recent is None else int(n_recent)
        self.exclude_seen = bool(exclude_seen)
        self._deg = np.diff(self.articles.ptr)
        self._rows = {}      # host neighbour rows, computed on demand
        self._dev = None     # (users_ptr, users_idx, articles_ptr, articles_idx) on one device
        self._table = None   # (nbr_id, nbr_count, nbr_score) on that device

    # ---- host form: the checker, independent of the device path --------------------------------------------------------
    def item_neighbors(self, item: int):
        """(ids int64[<= T], counts int64, scores float32) of one item row, best first."""
        item = int(item)
        if item not in self._rows:
            n_items = len(self.articles)
            reached, _ = self.users.gather(self.articles[item])         # every position of u in i's list x u's whole list
            c = np.bincount(reached, minlength=n_items)
            c[item] = 0
            ids = np.nonzero(c)[0]
            cnt = c[ids]
            if self.weighting == "cosine":
                sc = cnt.astype(np.float32) / np.sqrt(np.float32(self._deg[item]) * self._deg[ids].astype(np.float32))
            else:
                sc = cnt.astype(np.float32)
            key = cnt if self.weighting == "count" else sc            # raw counts order exactly, also beyond 2^24
            keep = np.lexsort((ids, -key.astype(np.float64)))[: self.neighbors]
            self._rows[item] = (ids[keep].astype(np.int64), cnt[keep].astype(np.int64), sc[keep].astype(np.float32))
        return self._rows[item]

    def scores_for(self, user_id: int):
        """(ids int64, r float32) of every item with r(u, j) > 0, best first; sums run in (list position, neighbour) order."""
        lst = self.users[user_id]
        taken = lst if self.n_recent is None else lst[-self.n_recent:]
        r = np.zeros(len(self.articles), dtype=np.float32)
        for a in taken:
            ids, _, sc = self.item_neighbors(int(a))
            r[ids] += sc                                                 # ids of one row are distinct
        if self.exclude_seen:
            r[lst] = 0
        ids = np.nonzero(r > 0)[0]
        order = np.lexsort((ids, -r[ids].astype(np.float64)))
        return ids[order].astype(np.int64), r[ids][order]

    def get_matches(self, user_id: int) -> Tensor:
        return t.from_numpy(self.scores_for(user_id)[0][: self.k].copy())

    def matches_for_all(self, num_users: int):
        out = np.full((num_users, self.k), -1, dtype=np.int64)
        for u in range(num_users):
            got = self.scores_for(u)[0][: self.k]
            out[u, : got.shape[0]] = got
        return out

    # ---- device form ---------------------------------------------------------------------------------------------------
    def _on(self, device):
        from .. import ops
        dev = t.device(device)
        if dev.type == "cuda" and dev.index is None:       # "cuda" and "cuda:0" are the same place: compare normalised devices
            dev = t.device("cuda", t.cuda.current_device())
        if self._dev is None or self._dev[0].device != dev:
            to32 = lambda a: t.from_numpy(np.ascontiguousarray(a.astype(np.int32))).to(dev)
            self._dev = (to32(self.users.ptr), to32(self.users.idx), to32(self.articles.ptr), to32(self.articles.idx))
            self._table = ops.cooc_item_neighbors(*self._dev, self.neighbors, self.weighting)
        return self._dev, self._table

    def item_neighbors_device(self, device):
        """(nbr_id int32[I, T], nbr_count int32[I, T], nbr_score float32[I, T]) on `device`, built once per device."""
        return self._on(device)[1]

    def matches_for_all_device(self, num_users: int, device, query_users=None, with_scores: bool = False):
        from .. import ops
        if num_users > len(self.users):
            raise IndexError(f"{num_users} query users but the purchase lists cover {len(self.users)}")
        (uptr, uidx, _, _), (nbr_id, _, nbr_score) = self._on(device)
        longest = int(np.diff(self.users.ptr).max()) if len(self.users) else 0
        out, score, cnt = ops.match_cooccurrence(uptr, uidx, nbr_id, nbr_score, self.k, n_queries=num_users,
                                                 query_users=query_users, n_recent=self.n_recent,
                                                 exclude_seen=self.exclude_seen, max_list_len=longest)
        return (out.to(t.int64), score, cnt) if with_scores else out.to(t.int64)


class RandomWalkMatcher(Matcher):
    """Random-walk (Pixie-style) candidates (include/laplace_hip.h, N3c, states the rule): num_walks walks of at most
    walk_length item -> user -> item traversals start at the user's last n_recent distinct items, an item's score is its
    visit count ("sum") or Pixie's multi-hit boost (sum_r sqrt(c_r))^2 over the start slots r ("multi_hit"), the k best by
    (score desc, id asc) are the proposals.  Nothing is trained and no table is built: the walks read the two adjacency
    lists, so an edge counts the moment it is in them, and the answer is a pure function of (graph, user, seed).

    The defaults are NOT tuned: they are the middle of the settings a numpy rehearsal tried, not the result of a search.
    Not in get_matchers: the reference has no such matcher, callers add it to their list themselves.

    There is no host form: the product may not import the test mirror (tests/random_walk_matcher_emulation.py), so
    get_matches and matches_for_all run the device call (get_matches for ONE query user, on the current GPU)."""

    def __init__(self, users_adj, articles_adj, k: int, *, num_walks: int = 256, walk_length: int = 4, restart_prob: float = 0.5,
                 n_recent: int = 8, boost: str = "multi_hit", exclude_seen: bool = False, seed: int = 0):
        from .. import ops
        ops.check_random_walks(k, num_walks, walk_length, restart_prob, n_recent, boost)
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 2 ** 64:
            raise ValueError(f"seed must be an integer in [0, 2^64), got {seed!r}")
        self.users = users_adj if isinstance(users_adj, AdjList) else AdjList(users_adj)
        self.articles = articles_adj if isinstance(articles_adj, AdjList) else AdjList(articles_adj)
        self.k, self.num_walks, self.walk_length = int(k), int(num_walks), int(walk_length)
        self.restart_prob, self.n_recent, self.boost = float(restart_prob), int(n_recent), boost
        self.exclude_seen, self.seed = bool(exclude_seen), int(seed)
        self._dev = None      # (articles_ptr, articles_idx, users_ptr, users_idx) on one device
        self._sorted = None   # the users' rows sorted by item id, on that device (exclude_seen only)

    def _on(self, device):
        from .. import ops
        dev = t.device(device)
        if dev.type == "cuda" and dev.index is None:       # "cuda" and "cuda:0" are the same place: compare normalised devices
            dev = t.device("cuda", t.cuda.current_device())
        if self._dev is None or self._dev[0].device != dev:
            to32 = lambda a: t.from_numpy(np.ascontiguousarray(a.astype(np.int32))).to(dev)
            self._dev = (to32(self.articles.ptr), to32(self.articles.idx), to32(self.users.ptr), to32(self.users.idx))
            self._sorted = ops.sort_csr_rows(self._dev[2], self._dev[3]) if self.exclude_seen else None
        return self._dev, self._sorted

    def matches_for_all_device(self, num_users: int, device, query_users=None, with_scores: bool = False):
        """int64 [n, k] with -1 pads for users 0 .. num_users - 1, or for query_users (ids, any order, repeats allowed) when
        given; with_scores: (ids, scores float32 [n, k] with 0 pads, counts int32 [n])."""
        from .. import ops
        if not 0 <= int(num_users) <= len(self.users):
            raise ValueError(f"num_users = {num_users} query users but the purchase lists cover {len(self.users)}")
        dev, ui_sorted = self._on(device)
        out, score, cnt = ops.match_random_walks(*dev, self.k, num_walks=self.num_walks, walk_length=self.walk_length,
                                                 restart_prob=self.restart_prob, n_recent=self.n_recent, boost=self.boost,
                                                 exclude_seen=self.exclude_seen, seed=self.seed, n_queries=int(num_users),
                                                 query_users=query_users, ui_sorted=ui_sorted)
        return (out.to(t.int64), score, cnt) if with_scores else out.to(t.int64)

    def matches_for_all(self, num_users: int):
        return self.matches_for_all_device(num_users, "cuda").cpu().numpy()

    def get_matches(self, user_id: int) -> Tensor:
        """The device call for this one user (there is no host form, see the class): needs a GPU."""
        if isinstance(user_id, bool) or not isinstance(user_id, (int, np.integer)) or not 0 <= int(user_id) < len(self.users):
            raise ValueError(f"user_id must be an integer in [0, {len(self.users)}), got {user_id!r}")
        row = self.matches_for_all_device(1, "cuda", query_users=[int(user_id)])[0].cpu()
        return row[row >= 0]


def get_matchers(dataset_type: str, users_adj, articles_adj, candidate_pool_size: int) -> List[Matcher]:
    """data/matching/__init__.py:9-24."""
    if dataset_type == "movielens":
        return [UsersWithCommonItemsMatcher(users_adj, articles_adj, candidate_pool_size)]
    if dataset_type == "fashion":
        return [PopularItemsMatcher.from_adjacency(articles_adj, candidate_pool_size),
                UsersWithCommonItemsMatcher(users_adj, articles_adj, candidate_pool_size)]
    raise ValueError("Unknown matchers type: {}".format(dataset_type))
