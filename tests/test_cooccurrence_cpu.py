"""ItemCooccurrenceMatcher on the host (the checker of the device path) against a dense A^T A reference written here, and
the C ABI's size queries and argument checks of the co-occurrence entry points — no GPU."""
import numpy as np
import pytest

U, A, E, REPEATS = 30, 25, 200, 20
EMPTY_USER, UNSOLD = 4, 9


def _graph(seed=0):
    """(users AdjList, articles AdjList, edge list) in shuffled transaction order: E distinct pairs + REPEATS repeated
    ones; user EMPTY_USER bought nothing, nobody bought item UNSOLD."""
    from laplace_amd.data.dataset import AdjList
    g = np.random.default_rng(seed)
    ok = np.array([k for k in range(U * A) if k // A != EMPTY_USER and k % A != UNSOLD])
    keys = g.choice(ok, size=E, replace=False)
    keys = np.concatenate([keys, g.choice(keys, size=REPEATS, replace=True)])
    g.shuffle(keys)
    u, a = keys // A, keys % A
    users, articles = {}, {}
    for x, y in zip(u.tolist(), a.tolist()):
        users.setdefault(x, []).append(y)
        articles.setdefault(y, []).append(x)
    return AdjList(users, U), AdjList(articles, A), u, a


def dense_reference(u, a, users, n_users, n_items, T, weighting, n_recent, exclude_seen):
    """r*[user, item] in float64 from the definitions: c = A^T A without its diagonal, s = c or c / sqrt(d_i d_j), each row
    cut to its T best by (s descending, j ascending), r = sum over the list positions taken."""
    M = np.zeros((n_users, n_items), dtype=np.int64)
    np.add.at(M, (u, a), 1)
    c = M.T @ M
    np.fill_diagonal(c, 0)
    d = M.sum(axis=0)
    if weighting == "cosine":
        s = c / np.sqrt(np.maximum(np.outer(d, d), 1).astype(np.float64))
        s32 = (c.astype(np.float32) / np.sqrt(np.maximum(np.outer(d, d), 1).astype(np.float32))).astype(np.float64)
    else:
        s = s32 = c.astype(np.float64)
    table = np.zeros_like(s)
    for i in range(n_items):
        nz = np.nonzero(c[i])[0]
        best = nz[np.lexsort((nz, -s32[i, nz]))][:T]     # the cut follows the float32 scores the matcher orders by
        table[i, best] = s[i, best]
    r = np.zeros((n_users, n_items))
    for x in range(n_users):
        lst = users[x]
        for it in (lst if n_recent is None else lst[-n_recent:]):
            r[x] += table[int(it)]
        if exclude_seen:
            r[x, lst] = 0
    return c, r


@pytest.mark.parametrize("weighting", ["count", "cosine"])
@pytest.mark.parametrize("n_recent", [None, 1, 3])
@pytest.mark.parametrize("exclude_seen", [False, True])
def test_get_matches_equals_dense_reference(weighting, n_recent, exclude_seen):
    from laplace_amd.data.matching import ItemCooccurrenceMatcher
    users, articles, u, a = _graph()
    T = 6
    c, r = dense_reference(u, a, users, U, A, T, weighting, n_recent, exclude_seen)
    for k in (1, 12, 100):
        m = ItemCooccurrenceMatcher(users, articles, k, neighbors=T, weighting=weighting, n_recent=n_recent,
                                    exclude_seen=exclude_seen)
        for x in range(U):
            got = m.get_matches(x).numpy()
            n_pos = int((r[x] > 0).sum())
            assert got.shape[0] == min(k, n_pos) and len(set(got.tolist())) == got.shape[0], (k, x)
            if exclude_seen:
                assert not np.isin(got, users[x]).any()
            if weighting == "count":   # exact: the order is pinned
                want = np.lexsort((np.arange(A), -r[x]))[: min(k, n_pos)]
                assert np.array_equal(got, want), (k, x)
            else:                      # float32 sums: near-ties may swap, nothing better may be left out
                tol = (len(users[x]) + 8) * 2.0 ** -23 * r[x].max()
                assert (r[x, got] > 0).all() and (np.diff(r[x, got]) <= tol).all(), (k, x)
                left = np.setdiff1d(np.arange(A), got)
                assert got.shape[0] == 0 or left.size == 0 or r[x, left].max() <= r[x, got].min() + tol, (k, x)
        assert m.get_matches(EMPTY_USER).numel() == 0                       # no purchases: no proposals
        assert np.array_equal(m.matches_for_all(U)[EMPTY_USER], np.full(k, -1))
    ids, cnt, sc = m.item_neighbors(UNSOLD)                                 # an item nobody bought has no neighbours ...
    assert ids.size == 0 and cnt.size == 0 and sc.size == 0
    for i in range(A):                                                      # ... and is nobody's neighbour; counts are exact
        ids, cnt, _ = m.item_neighbors(i)
        assert UNSOLD not in ids and i not in ids and np.array_equal(cnt, c[i, ids])
        assert ids.size == min(T, int((c[i] > 0).sum()))


def test_matches_for_all_equals_get_matches():
    from laplace_amd.data.matching import ItemCooccurrenceMatcher
    users, articles, _, _ = _graph(1)
    m = ItemCooccurrenceMatcher(users, articles, 7, neighbors=4, weighting="count", exclude_seen=True)
    allm = m.matches_for_all(U)
    assert allm.shape == (U, 7) and allm.dtype == np.int64
    for x in range(U):
        want = m.get_matches(x).numpy()
        assert np.array_equal(allm[x, : want.size], want) and (allm[x, want.size:] == -1).all()


def test_constructor_refuses_bad_arguments():
    from laplace_amd.data.matching import ItemCooccurrenceMatcher
    users, articles, _, _ = _graph()
    for kw in (dict(neighbors=0), dict(neighbors=65), dict(weighting="jaccard"), dict(n_recent=0)):
        with pytest.raises(ValueError):
            ItemCooccurrenceMatcher(users, articles, 5, **kw)
    with pytest.raises(ValueError):
        ItemCooccurrenceMatcher(users, articles, 0)


def test_get_matchers_is_unchanged():
    from laplace_amd.data.matching import ItemCooccurrenceMatcher, get_matchers
    users, articles, _, _ = _graph()
    for kind in ("movielens", "fashion"):
        assert not any(isinstance(m, ItemCooccurrenceMatcher) for m in get_matchers(kind, users, articles, 5))


def test_size_queries_and_argument_checks_run_without_gpu():
    from laplace_amd import _lib
    L = _lib.lib()
    assert L.mi_cooc_items_workspace_bytes(100, 1000, 32) > 0
    assert L.mi_match_cooc_workspace_bytes(100, 50, 32) > 0
    for nnz in (0, 1000, 10 ** 6, 2 ** 31 - 1):
        for T in (1, 8, 32, 64):
            assert L.mi_cooc_items_workspace_bytes(105542, nnz, T) >= L.mi_cooc_items_workspace_bytes(105542, max(nnz - 1, 0), T) > 0
    sizes = [L.mi_match_cooc_workspace_bytes(1000, 2000, T) for T in (1, 8, 32, 64)]    # sized by the queries, the longest list and T
    assert sizes[0] > 0 and sizes == sorted(sizes)
    sizes = [L.mi_cooc_items_workspace_bytes(105542, 10 ** 6, T) for T in (1, 8, 32, 64)]
    assert sizes[0] > 0 and sizes == sorted(sizes)
    assert L.mi_match_cooc_workspace_bytes(1000, 4000, 32) >= L.mi_match_cooc_workspace_bytes(1000, 2000, 32)
    assert L.mi_match_cooc_workspace_bytes(2000, 2000, 32) >= L.mi_match_cooc_workspace_bytes(1000, 2000, 32)
    # what the calls refuse has no size
    assert L.mi_cooc_items_workspace_bytes(100, 1000, 0) == 0 and L.mi_cooc_items_workspace_bytes(100, 1000, 65) == 0
    assert L.mi_cooc_items_workspace_bytes(100, 2 ** 31, 32) == 0 and L.mi_cooc_items_workspace_bytes(-1, 0, 32) == 0
    assert L.mi_match_cooc_workspace_bytes(100, 50, 0) == 0 and L.mi_match_cooc_workspace_bytes(-1, 50, 32) == 0
    # MI_ERR_BAD_ARG before any launch: null pointers, T outside 1..64, an unknown weighting, nnz >= 2^31, k <= 0
    BAD, fake = -1, 256   # never dereferenced: the checks come first
    assert L.mi_cooc_items_topt(10, 10, 20, None, None, None, None, 32, 0, None, None, None, None, 0, None) == BAD
    for T in (0, -3, 65):
        assert L.mi_cooc_items_topt(10, 10, 20, fake, fake, fake, fake, T, 0, fake, fake, fake, fake, 1 << 20, None) == BAD
    assert L.mi_cooc_items_topt(10, 10, 20, fake, fake, fake, fake, 32, 7, fake, fake, fake, fake, 1 << 20, None) == BAD
    assert L.mi_cooc_items_topt(10, 10, 2 ** 31, fake, fake, fake, fake, 32, 0, fake, fake, fake, fake, 1 << 20, None) == BAD
    assert L.mi_cooc_items_topt(10, 10, 20, fake, fake, fake, fake, 32, 0, fake, fake, fake, fake, 8, None) == _lib.MI_ERR_WORKSPACE
    assert L.mi_match_cooc_i32(5, None, None, None, 10, 32, None, None, 12, 0, 0, None, None, None, None, 0, None) == BAD
    for k in (0, -1):
        assert L.mi_match_cooc_i32(5, None, fake, fake, 10, 32, fake, fake, k, 0, 0, fake, fake, fake, fake, 1 << 20, None) == BAD
    for T in (0, 65):
        assert L.mi_match_cooc_i32(5, None, fake, fake, 10, T, fake, fake, 12, 0, 0, fake, fake, fake, fake, 1 << 20, None) == BAD
    assert L.mi_match_cooc_i32(5, None, fake, fake, 10, 32, fake, fake, 12, 0, 0, fake, None, None, fake, 8, None) == _lib.MI_ERR_WORKSPACE
