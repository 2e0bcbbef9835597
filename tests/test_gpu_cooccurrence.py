"""GPU: the scored item co-occurrence matcher (csrc/cooccurrence.hip: mi_cooc_items_topt, mi_match_cooc_i32) against NumPy
references written here.  Counts are integer work and must be exact; float32 cosine scores go through the tolerant check
below, whose bound is derived from the float32 format, not measured:

  tol = (n_terms + 8) * 2^-23 * r*    (r* the float64 reference score, n_terms the terms summed for the row; 0 in stage 1)

every term is positive (relative errors do not amplify), carries at most four roundings (multiply, sqrt, divide, the
conversion of c or d) and every partial sum adds one rounding of 2^-24; the bound is that, doubled."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch as t

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 2.0 ** -23


# ---- graphs --------------------------------------------------------------------------------------------------------------
def _from_edges(u, a, U, A):
    from laplace_amd.data.dataset import AdjList
    return AdjList.from_edges(u, a, U), AdjList.from_edges(a, u, A)     # stable: both keep the transaction order


def _small_graph(seed=0, U=300, A=90, E=2500, empty_users=(0, 7, 299), unsold=33, repeats=100):
    g = np.random.default_rng(seed)
    ok = np.array([k for k in range(U * A) if k % A != unsold and k // A not in empty_users])
    keys = g.choice(ok, size=E, replace=False)
    keys = np.concatenate([keys, g.choice(keys, size=repeats, replace=True)])   # repeated purchases
    g.shuffle(keys)                                                            # list order = transaction order, not sorted
    u, a = keys // A, keys % A
    return _from_edges(u, a, U, A) + (u, a, U, A)


HUB_ITEM, HUB_USER, ONE_ITEM_USER = 41234, 17, 5     # the hub item lies in the SECOND band of 36 864 ids


def _big_graph():
    """I = 70 000 (4 I bytes exceed a CU's LDS: two bands), U = 4 000, ~60 000 edges; HUB_ITEM is held by every user (its
    expansion is every edge), HUB_USER holds 3 000 distinct items (192 000 stage-2 terms at T = 64), ONE_ITEM_USER holds
    the hub item only."""
    U, A = 4000, 70000
    g = np.random.default_rng(7)
    deg = g.integers(4, 24, U)
    u = np.repeat(np.arange(U), deg)
    a = (A * g.random(u.size) ** 3).astype(np.int64)               # skewed towards low ids: real co-occurrence
    keep = (u != HUB_USER) & (u != ONE_ITEM_USER) & (a != HUB_ITEM)
    u, a = u[keep], a[keep]
    hub_items = g.choice(np.setdiff1d(np.arange(A), [HUB_ITEM]), size=2999, replace=False)
    u = np.concatenate([u, np.full(2999, HUB_USER), np.arange(U)])
    a = np.concatenate([a, hub_items, np.full(U, HUB_ITEM)])
    p = g.permutation(u.size)
    u, a = u[p], a[p]
    return _from_edges(u, a, U, A) + (u, a, U, A)


# ---- references ------------------------------------------------------------------------------------------------------------
class Ref:
    """c(i, j) for every pair with c > 0, from np.unique over i * I + j keys of the two-hop walks (no dense matrix)."""

    def __init__(self, users, articles, n_items):
        self.I, self._s64 = n_items, {}
        self.d = np.diff(articles.ptr)
        per_edge_user = np.repeat(np.arange(len(users)), np.diff(users.ptr))       # the user of every entry of users.idx
        j, cnt = users.gather(per_edge_user)                                        # each entry x the user's whole list
        i = np.repeat(users.idx, cnt)
        keys = (i * n_items + j)[i != j]
        self.keys, self.c = np.unique(keys, return_counts=True)
        self.i, self.j = self.keys // n_items, self.keys % n_items
        self.row_nnz = np.bincount(self.i, minlength=n_items)

    def score64(self, weighting):
        if weighting not in self._s64:   # computed once: the references are shared and left unchanged
            self._s64[weighting] = (self.c.astype(np.float64) if weighting == "count" else
                                    self.c / np.sqrt(self.d[self.i].astype(np.float64) * self.d[self.j]))
        return self._s64[weighting]

    def table(self, T, weighting):
        """(ids, counts) int64 [I, T] by (s descending, j ascending) on exact float64 scores, -1 / 0 padded."""
        s = self.score64(weighting)
        order = np.lexsort((self.j, -s, self.i))
        start = np.concatenate([[0], np.cumsum(self.row_nnz)])
        rank = np.arange(order.size) - start[self.i[order]]
        keep = rank < T
        ids = np.full((self.I, T), -1, dtype=np.int64)
        cnt = np.zeros((self.I, T), dtype=np.int64)
        ids[self.i[order][keep], rank[keep]] = self.j[order][keep]
        cnt[self.i[order][keep], rank[keep]] = self.c[order][keep]
        return ids, cnt

    def lookup(self, rows, ids):
        """(found, position in self.keys) of the pairs (rows, ids)."""
        k = rows * self.I + ids
        pos = np.minimum(np.searchsorted(self.keys, k), self.keys.size - 1)
        return self.keys[pos] == k, pos


def check_stage1(ref: Ref, T, weighting, ids, cnt, sc):
    ids, cnt, sc = ids.cpu().numpy().astype(np.int64), cnt.cpu().numpy().astype(np.int64), sc.cpu().numpy()
    assert ids.shape == (ref.I, T) and cnt.shape == (ref.I, T) and sc.shape == (ref.I, T)
    n_row = np.minimum(ref.row_nnz, T)
    valid = np.arange(T)[None, :] < n_row[:, None]
    assert ((ids >= 0) == valid).all(), "row length = min(T, neighbours with c > 0), -1 padded"
    assert (cnt[~valid] == 0).all() and (sc[~valid] == 0).all()
    if weighting == "count":   # exact keys: the table is pinned
        want_ids, want_cnt = ref.table(T, "count")
        assert np.array_equal(ids, want_ids) and np.array_equal(cnt, want_cnt)
        assert np.array_equal(sc, want_cnt.astype(np.float32))
        return
    rows = np.broadcast_to(np.arange(ref.I)[:, None], ids.shape)[valid]
    found, pos = ref.lookup(rows, ids[valid])
    assert found.all(), "every returned id has c > 0 (and is not the row itself)"
    assert np.array_equal(cnt[valid], ref.c[pos]), "counts are exact whatever the weighting"
    srt = np.sort(np.where(valid, ids, np.arange(T)[None, :] + ref.I), axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all(), "ids of a row are distinct"
    s = ref.score64("cosine")
    s_ret = np.zeros(ids.shape)
    s_ret[valid] = s[pos]
    assert (np.abs(sc[valid] - s_ret[valid]) <= 8 * EPS * s_ret[valid]).all(), float(np.abs(sc[valid] / s_ret[valid] - 1).max())
    both = valid[:, 1:]
    assert (s_ret[:, 1:][both] <= (s_ret[:, :-1] * (1 + 8 * EPS))[both]).all(), "r* non-increasing along the row, to within tol"
    floor = np.where(valid, s_ret, np.inf).min(axis=1)                       # smallest returned r* per row
    above = s > floor[ref.i] * (1 + 8 * EPS)                                 # reference pairs clearly better than it ...
    n_above = np.bincount(ref.i[above], minlength=ref.I)
    n_ret_above = (np.where(valid, s_ret, 0) > (floor * (1 + 8 * EPS))[:, None]).sum(axis=1)
    assert np.array_equal(n_above, n_ret_above), "... are all in the row: nothing better was left out"


def stage2_reference(ref: Ref, weighting, users, nbr_id, user, n_recent, exclude_seen):
    """(r* float64 [I], n_terms) from the neighbour ids the device kept and their exact float64 scores."""
    lst = users[user]
    taken = lst if n_recent is None else lst[-n_recent:]
    r = np.zeros(ref.I)
    if taken.size == 0:
        return r, 0
    ids = nbr_id[taken]                                   # [n, T]
    ok = ids >= 0
    rows = np.broadcast_to(taken[:, None], ids.shape)[ok]
    found, pos = ref.lookup(rows, ids[ok])
    assert found.all()
    np.add.at(r, ids[ok], ref.score64(weighting)[pos])
    if exclude_seen:
        r[lst] = 0
    return r, int(ok.sum())


def check_stage2_row(r, n_terms, k, lst, exclude_seen, got_ids, got_sc, got_n, exact):
    n_pos = int((r > 0).sum())
    n = min(k, n_pos)
    assert got_n == n and (got_ids[n:] == -1).all() and (got_sc[n:] == 0).all(), (got_n, n)
    ids = got_ids[:n]
    if exact:   # integer-valued sums below 2^24: the order is pinned
        want = np.lexsort((np.arange(r.size), -r))[:n]
        assert np.array_equal(ids, want) and np.array_equal(got_sc[:n].astype(np.float64), r[want])
        return
    assert ((ids >= 0) & (ids < r.size)).all() and np.unique(ids).size == n and (r[ids] > 0).all()
    if exclude_seen:
        assert not np.isin(ids, lst).any()
    tol = (n_terms + 8) * EPS
    assert (np.abs(got_sc[:n] - r[ids]) <= tol * r[ids]).all()
    assert (r[ids][1:] <= r[ids][:-1] * (1 + tol)).all()
    if 0 < n < n_pos:
        rest = r.copy()
        rest[ids] = 0
        assert rest.max() <= r[ids].min() * (1 + tol)


# ---- shared state: graphs, references and device tables are built once ---------------------------------------------------
@pytest.fixture(scope="module")
def small():
    users, articles, u, a, U, A = _small_graph()
    return SimpleNamespace(users=users, articles=articles, U=U, A=A, ref=Ref(users, articles, A))


@pytest.fixture(scope="module")
def big():
    users, articles, u, a, U, A = _big_graph()
    return SimpleNamespace(users=users, articles=articles, U=U, A=A, ref=Ref(users, articles, A))


def _dev_csr(g):
    to32 = lambda x: t.from_numpy(np.ascontiguousarray(x.astype(np.int32))).to(DEV)
    return to32(g.users.ptr), to32(g.users.idx), to32(g.articles.ptr), to32(g.articles.idx)


# ---- 1. exactness ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighting", ["count", "cosine"])
@pytest.mark.parametrize("T", [1, 8, 64])
def test_neighbor_table_equals_reference(small, T, weighting):
    from laplace_amd import ops
    assert small.ref.row_nnz[33] == 0
    ids, cnt, sc = ops.cooc_item_neighbors(*_dev_csr(small), T, weighting)
    check_stage1(small.ref, T, weighting, ids, cnt, sc)
    assert bool((ids[33] == -1).all())                    # the article nobody bought has no neighbours


@pytest.mark.parametrize("n_recent,exclude_seen", [(None, False), (None, True), (1, True), (5, False)])
@pytest.mark.parametrize("k", [1, 12, 257])
def test_device_candidates_equal_get_matches(small, k, n_recent, exclude_seen):
    from laplace_amd.data.matching import ItemCooccurrenceMatcher
    m = ItemCooccurrenceMatcher(small.users, small.articles, k, neighbors=8, weighting="count", n_recent=n_recent,
                                exclude_seen=exclude_seen)
    g = np.random.default_rng(k)
    subset = g.permutation(small.U)[:120]
    subset[7] = subset[3]                                # a repeated id
    subset[11] = 299                                     # a user without purchases
    for query in (None, subset):
        q = None if query is None else t.from_numpy(query).to(DEV)
        n = small.U if query is None else query.size
        got, sc, cnt = m.matches_for_all_device(n, DEV, query_users=q, with_scores=True)
        assert got.shape == (n, k) and got.dtype == t.int64 and sc.shape == (n, k) and cnt.shape == (n,)
        got, cnt = got.cpu(), cnt.cpu()
        for row in range(n):
            want = m.get_matches(int(row if query is None else query[row]))
            assert t.equal(got[row, : want.numel()], want), row
            assert bool((got[row, want.numel():] == -1).all()) and int(cnt[row]) == want.numel(), row   # k = 257: padded
    assert int(cnt[11]) == 0


@pytest.mark.parametrize("n_recent,exclude_seen", [(None, True), (5, False)])
def test_cosine_candidates_pass_the_tolerant_check(small, n_recent, exclude_seen):
    from laplace_amd import ops
    uptr, uidx, aptr, aidx = _dev_csr(small)
    nbr_id, nbr_cnt, nbr_sc = ops.cooc_item_neighbors(uptr, uidx, aptr, aidx, 8, "cosine")
    nbr = nbr_id.cpu().numpy().astype(np.int64)
    for k in (12, 257):
        ids, sc, cnt = (x.cpu().numpy() for x in ops.match_cooccurrence(uptr, uidx, nbr_id, nbr_sc, k, n_recent=n_recent,
                                                                        exclude_seen=exclude_seen))
        for user in range(small.U):
            r, n_terms = stage2_reference(small.ref, "cosine", small.users, nbr, user, n_recent, exclude_seen)
            check_stage2_row(r, n_terms, k, small.users[user], exclude_seen, ids[user], sc[user], int(cnt[user]), exact=False)


# ---- 2. sizes that break a naive kernel, then the small graph again on the same workspaces -------------------------------
def test_two_bands_hub_row_and_hub_user_then_small_graph_on_same_workspace(big, small):
    from laplace_amd import ops
    T, k = 64, 50
    assert 4 * big.A > 160 * 1024 and big.ref.d[HUB_ITEM] == big.U and np.diff(big.users.ptr)[HUB_USER] == 3000
    assert np.diff(big.users.ptr)[ONE_ITEM_USER] == 1
    uptr, uidx, aptr, aidx = _dev_csr(big)
    nbr_id, nbr_cnt, nbr_sc = ops.cooc_item_neighbors(uptr, uidx, aptr, aidx, T, "count")
    check_stage1(big.ref, T, "count", nbr_id, nbr_cnt, nbr_sc)                 # counts exact, hub row included
    assert int(nbr_cnt[HUB_ITEM].sum()) > 0 and int((nbr_id[HUB_ITEM] >= 0).sum()) == T
    g = np.random.default_rng(3)
    query = np.concatenate([[HUB_USER, ONE_ITEM_USER], g.choice(big.U, size=200, replace=False)])
    nbr = nbr_id.cpu().numpy().astype(np.int64)
    for exclude_seen in (False, True):
        ids, sc, cnt = (x.cpu().numpy() for x in ops.match_cooccurrence(uptr, uidx, nbr_id, nbr_sc, k,
                                                                        query_users=t.from_numpy(query).to(DEV),
                                                                        exclude_seen=exclude_seen))
        for row, user in enumerate(query.tolist()):
            r, n_terms = stage2_reference(big.ref, "count", big.users, nbr, user, None, exclude_seen)
            assert r.max() < 2 ** 24
            check_stage2_row(r, n_terms, k, big.users[user], exclude_seen, ids[row], sc[row], int(cnt[row]), exact=True)
    ws_before = {key: w.data_ptr() for key, w in ops._COOC_WS.items()}
    # second call, same workspaces, another graph: stale counters or a stale running top-T would show here
    s_ids, s_cnt, s_sc = ops.cooc_item_neighbors(*_dev_csr(small), 8, "count")
    check_stage1(small.ref, 8, "count", s_ids, s_cnt, s_sc)
    suptr, suidx, _, _ = _dev_csr(small)
    ids, sc, cnt = (x.cpu().numpy() for x in ops.match_cooccurrence(suptr, suidx, s_ids, s_sc, 12, exclude_seen=True))
    s_nbr = s_ids.cpu().numpy().astype(np.int64)
    for user in range(small.U):
        r, n_terms = stage2_reference(small.ref, "count", small.users, s_nbr, user, None, True)
        check_stage2_row(r, n_terms, 12, small.users[user], True, ids[user], sc[user], int(cnt[user]), exact=True)
    assert {key: w.data_ptr() for key, w in ops._COOC_WS.items()} == ws_before   # the workspaces were reused, not regrown


# ---- 3. quality on the planted graph ---------------------------------------------------------------------------------------
def test_recall_on_planted_graph_beats_popularity():
    """NumPy statement of the definitions on this graph: recall@12 0.395 against 0.171 for the 12 most popular items (2.3 x);
    the 1.5 x asked for leaves room for tie order only — counts are exact, nothing else can move."""
    from laplace_amd import synthetic as S
    from laplace_amd.data.matching import ItemCooccurrenceMatcher, PopularItemsMatcher
    spec = S.SyntheticSpec(2000, 600, 30000, seed=5, deg_min=2, deg_max=200, communities=8)
    ei = S.generate(spec)
    held = S.heldout_edges(spec, ei, 1000)
    users, articles = _from_edges(ei[0].numpy(), ei[1].numpy(), spec.num_users, spec.num_items)
    m = ItemCooccurrenceMatcher(users, articles, 12, neighbors=32, weighting="cosine", exclude_seen=True)
    got = m.matches_for_all_device(held.shape[1], DEV, query_users=held[0].to(DEV)).cpu()
    recall = float((got == held[1][:, None]).any(dim=1).float().mean())
    pop = PopularItemsMatcher.from_adjacency(articles, 12).get_matches(0)
    recall_pop = float(t.isin(held[1], pop).float().mean())
    print(f"recall@12: co-occurrence {recall:.4f}, popular {recall_pop:.4f}")
    assert recall >= 1.5 * recall_pop, (recall, recall_pop)


# ---- 4. determinism --------------------------------------------------------------------------------------------------------
def test_two_calls_are_bit_identical(big):
    from laplace_amd import ops
    uptr, uidx, aptr, aidx = _dev_csr(big)
    first = ops.cooc_item_neighbors(uptr, uidx, aptr, aidx, 64, "cosine")
    second = ops.cooc_item_neighbors(uptr, uidx, aptr, aidx, 64, "cosine")
    for x, y in zip(first, second):
        assert t.equal(x, y)
    check_stage1(big.ref, 64, "cosine", *first)
    q = t.arange(0, big.U, 7, device=DEV)                 # HUB_USER = 17 is not a multiple of 7 ...
    q = t.cat([q, t.tensor([HUB_USER, ONE_ITEM_USER], device=DEV)])   # ... so add it: the workspace path is covered
    a = ops.match_cooccurrence(uptr, uidx, first[0], first[2], 20, query_users=q, exclude_seen=True)
    a = [x.clone() for x in a]
    b = ops.match_cooccurrence(uptr, uidx, first[0], first[2], 20, query_users=q, exclude_seen=True)
    for x, y in zip(a, b):
        assert t.equal(x, y)
    nbr = first[0].cpu().numpy().astype(np.int64)
    ids, sc, cnt = (x.cpu().numpy() for x in a)
    for row in (q.numel() - 2, q.numel() - 1, 0, 100):    # the hub user's 192 000 float terms, the one-item user, two others
        user = int(q[row])
        r, n_terms = stage2_reference(big.ref, "cosine", big.users, nbr, user, None, True)
        check_stage2_row(r, n_terms, 20, big.users[user], True, ids[row], sc[row], int(cnt[row]), exact=False)


# ---- 5. plumbing -----------------------------------------------------------------------------------------------------------
class HostOnly:  # hides the device form: forces candidate_csr's host path
    def __init__(self, m):
        self.m = m

    def get_matches(self, u):
        return self.m.get_matches(u)


def test_candidate_csr_device_equals_host(small):
    from laplace_amd.data.device_sampler import candidate_csr, candidate_csr_device
    from laplace_amd.data.matching import ItemCooccurrenceMatcher, PopularItemsMatcher
    ms = [PopularItemsMatcher.from_adjacency(small.articles, 10),
          ItemCooccurrenceMatcher(small.users, small.articles, 15, neighbors=8, weighting="count")]
    ptr_h, idx_h = candidate_csr(ms, small.U)
    ptr_x, idx_x = candidate_csr([HostOnly(m) for m in ms], small.U)
    ptr_d, idx_d = candidate_csr_device(ms, small.U, DEV)
    assert np.array_equal(ptr_h, ptr_x) and np.array_equal(idx_h, idx_x)
    assert np.array_equal(ptr_d.cpu().numpy(), ptr_h) and np.array_equal(idx_d.cpu().numpy(), idx_h)
    table = ms[1].item_neighbors_device(DEV)
    assert table[0].shape == (small.A, 8) and ms[1].item_neighbors_device(DEV)[0].data_ptr() == table[0].data_ptr()   # built once


def test_evaluation_sampler_builds_the_same_candidates_both_ways():
    from laplace_amd import synthetic as S
    from laplace_amd.data.device_sampler import DeviceGraphSampler
    from laplace_amd.data.matching import ItemCooccurrenceMatcher, PopularItemsMatcher
    spec = S.SyntheticSpec(400, 150, 5000, seed=11, deg_min=1, deg_max=80)
    graph, users, articles = S.generate_hetero(spec, customer_cards=(50, 2, 84), article_cards=(40, 9))
    cfg = SimpleNamespace(k=12, num_neighbors=8, n_hop_neighbors=2, positive_edges_ratio=0.5, negative_edges_ratio=3.0, batch_size=16)
    ms = [PopularItemsMatcher.from_adjacency(articles, 10),
          ItemCooccurrenceMatcher(users, articles, 10, neighbors=16, weighting="count", exclude_seen=True)]
    a = DeviceGraphSampler(cfg, graph, users, articles, batch_size=16, randomization=False, device=DEV, seed=3, train=False, matchers=ms)
    b = DeviceGraphSampler(cfg, graph, users, articles, batch_size=16, randomization=False, device=DEV, seed=3, train=False,
                           matchers=[HostOnly(m) for m in ms])
    assert t.equal(a.cptr.cpu(), b.cptr.cpu()) and t.equal(a.cidx.cpu(), b.cidx.cpu())
