"""The random-walk matcher (include/laplace_hip.h, N3c) without a GPU: the laws of the CPU mirror of the rule
(tests/random_walk_matcher_emulation.py) on a graph whose answer can be written down and on the shared test graph, every
ValueError of ops.match_random_walks / RandomWalkMatcher / RandomWalkRecommender, and the argument checks of
mi_match_random_walks_i32 (they return before anything touches a device)."""
import numpy as np
import pytest
import torch as t

import random_walk_matcher_emulation as WE
from oracle import pinsage_ref as PR

GOOD = dict(num_walks=8, walk_length=2, restart_prob=0.5, n_recent=4, boost="sum")
BAD = [("num_walks", 0), ("num_walks", -3), ("num_walks", 2.5), ("walk_length", 0), ("restart_prob", 1.0), ("restart_prob", -0.1),
       ("restart_prob", float("nan")), ("n_recent", 0), ("n_recent", 17), ("n_recent", 2.0), ("boost", "max"), ("boost", None),
       ("num_walks", 4097)]   # 4097 * 2 visits: above the limit


def test_draw_layout_is_the_oracles():
    WE.assert_layout_is_the_oracles()


# ---- a graph whose answer can be written down --------------------------------------------------------------------------------
# Every item is held by ONE user, so every hop returns to the walker's own row: user 0 holds item 3 three times and nothing
# else (every traversal ends at 3), user 1 holds nothing, user 2 holds items 1 and 2 (the walks never leave {1, 2}); item 0 is
# unsold.
def _forced():
    rows = [[3, 3, 3], [], [1, 2]]
    u = np.array([q for q, r in enumerate(rows) for _ in r], dtype=np.int64)
    a = np.array([i for r in rows for i in r], dtype=np.int64)
    return WE.csr_pair(u, a, 3, 4)


@pytest.mark.parametrize("W,L", [(1, 1), (7, 3), (64, 2), (1024, 4)])
def test_forced_walks(W, L):
    icsr, ucsr = _forced()
    n = W * L                                                     # restart_prob 0: every walk makes all L traversals
    for boost, want in (("sum", np.float32(n)), ("multi_hit", np.float32(WE.ROOTS[n] * WE.ROOTS[n]))):
        rule = WE.Rule(W, L, 0.0, 16, boost, False)
        ids, sc, cnt = WE.match([0, 1, 2], icsr, ucsr, rule, 3, seed=5)
        assert ids[0].tolist() == [3, -1, -1] and sc[0].tolist() == [want, 0, 0] and cnt[0] == 1
        assert ids[1].tolist() == [-1, -1, -1] and sc[1].tolist() == [0, 0, 0] and cnt[1] == 0      # an empty row: no proposal
        assert set(ids[2][ids[2] >= 0].tolist()) <= {1, 2} and cnt[2] == int((ids[2] >= 0).sum()) >= 1
        if boost == "sum":
            assert float(sc[2].sum()) == n
        ids, sc, cnt = WE.match([0, 1, 2], icsr, ucsr, WE.Rule(W, L, 0.0, 16, boost, True), 3, seed=5)
        assert (ids == -1).all() and (sc == 0).all() and (cnt == 0).all()                           # nothing outside the own row
    # L = 1 never tests for a restart: restart_prob does not matter
    a = WE.match([0, 2], icsr, ucsr, WE.Rule(W, 1, 0.0, 16, "sum", False), 3, seed=5)
    b = WE.match([0, 2], icsr, ucsr, WE.Rule(W, 1, 0.9, 16, "sum", False), 3, seed=5)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and float(a[1][0, 0]) == W


# ---- the shared graph ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def graph():
    u, a = WE.small_graph()
    return WE.csr_pair(u, a, WE.N_USERS, WE.N_ITEMS)


def test_shared_graph_has_the_special_rows(graph):
    icsr, ucsr = graph
    assert all(len(ucsr[u]) == 0 for u in WE.EMPTY_USERS) and len(icsr[WE.UNSOLD]) == 0
    assert ucsr[WE.LONE_USER].tolist() == [WE.LONE_ITEM] and icsr[WE.LONE_ITEM].tolist() == [WE.LONE_USER]
    assert len(ucsr[WE.DUP_USER]) == 150 and len(set(ucsr[WE.DUP_USER].tolist())) <= 10
    assert len(ucsr[WE.LONG_USER]) == 3000


@pytest.mark.parametrize("W,L,p,n_recent", [(7, 3, 0.5, 3), (33, 5, 0.0, 16), (64, 2, 0.5, 1), (256, 4, 0.5, 8)])
def test_counts_sum_to_the_traversal_ends(graph, W, L, p, n_recent):
    """Every user a hop reaches holds an item (the lists are transposes), so a walk ends by its restart draw alone: the number
    of traversal ends is known from the third words of the draws."""
    icsr, ucsr = graph
    rule = WE.Rule(W, L, p, n_recent, "sum", False)
    thr = int(p * 4294967296.0)
    for u in (1, 2, 150, WE.LONE_USER, WE.DUP_USER, WE.LONG_USER) + WE.EMPTY_USERS:
        counts = WE.slot_counts(u, icsr, ucsr, rule, seed=9, step=3)
        if u in WE.EMPTY_USERS:
            assert counts == []
            continue
        w2 = WE._walk_words(W * L, u, 9, 3)[2]
        ends = 0
        for w in range(W):
            n = 1
            while n < L and w2[w * L + n] >= thr:
                n += 1
            ends += n
        assert sum(sum(c.values()) for c in counts) == ends
        R = len(counts)
        assert R == min(n_recent, len(set(ucsr[u].tolist()[-64:])))
        for r, c in enumerate(counts):                       # walk w belongs to slot w % R
            assert sum(c.values()) >= len(range(r, W, R))    # at least its first traversal
        ids, sc, cnt = WE.match_user(u, icsr, ucsr, rule, 200, 9, 3, counts=counts)
        assert float(sc.sum()) == ends and cnt == int((ids >= 0).sum()) == len(set().union(*counts))
        assert all((sc[i], -ids[i]) >= (sc[i + 1], -ids[i + 1]) for i in range(cnt - 1))      # score desc, id asc


def test_boosts_agree_on_one_slot_and_differ_on_many(graph):
    icsr, ucsr = graph
    users = [1, 2, 50, 150, WE.DUP_USER, WE.LONG_USER]
    one = [WE.match(users, icsr, ucsr, WE.Rule(256, 4, 0.5, 1, b, False), 200, seed=1) for b in ("sum", "multi_hit")]
    assert np.array_equal(one[0][0], one[1][0]) and np.array_equal(one[0][2], one[1][2])   # sqrt is monotone: the same order
    many = [WE.match(users, icsr, ucsr, WE.Rule(256, 4, 0.5, 16, b, False), 200, seed=1) for b in ("sum", "multi_hit")]
    assert np.array_equal(many[0][2], many[1][2]) and not np.array_equal(many[0][0], many[1][0])   # the boost reorders


def test_exclude_seen_drops_the_whole_row(graph):
    icsr, ucsr = graph
    for u in (2, WE.DUP_USER, WE.LONG_USER, WE.LONE_USER):
        ids, _, cnt = WE.match_user(u, icsr, ucsr, WE.Rule(256, 4, 0.5, 3, "multi_hit", True), 200, seed=4)
        assert not np.isin(ids[ids >= 0], ucsr[u]).any()
        assert (cnt == 0) == (u == WE.LONE_USER)


# ---- refusals: ValueError naming the argument, without a device --------------------------------------------------------------
def _cpu_csr():
    u, a = WE.small_graph()
    icsr, ucsr = WE.csr_pair(u, a, WE.N_USERS, WE.N_ITEMS)
    to32 = lambda x: t.from_numpy(x.astype(np.int32))
    return to32(icsr.ptr), to32(icsr.idx), to32(ucsr.ptr), to32(ucsr.idx)


@pytest.mark.parametrize("name,value", BAD + [("k", 0), ("k", -1)])
def test_ops_refuses_by_name(name, value):
    from laplace_amd import ops
    kw = dict(GOOD, exclude_seen=False, seed=0)
    k = 5
    if name == "k":
        k = value
    else:
        kw[name] = value
    with pytest.raises(ValueError, match="num_walks" if value == 4097 else name):
        ops.match_random_walks(*_cpu_csr(), k, **kw)


def test_ops_refuses_host_query_ids_and_counts():
    from laplace_amd import _lib, ops
    csr, kw = _cpu_csr(), dict(GOOD, exclude_seen=False, seed=0)
    for q in ([0, WE.N_USERS], [-1], np.array([5, 10 ** 9]), t.tensor([WE.N_USERS])):
        with pytest.raises(ValueError, match="query_users"):
            ops.match_random_walks(*csr, 5, query_users=q, **kw)
    for n in (-1, WE.N_USERS + 1):
        with pytest.raises(ValueError, match="n_queries"):
            ops.match_random_walks(*csr, 5, n_queries=n, **kw)
    with pytest.raises(ValueError, match="seed"):
        ops.match_random_walks(*csr, 5, **dict(kw, seed=-1))
    with pytest.raises(_lib.MiError, match="no CPU fallback"):      # valid arguments on CPU tensors: an error, not a slow path
        ops.match_random_walks(*csr, 5, **kw)


@pytest.mark.parametrize("name,value", BAD + [("k", 0), ("seed", -1), ("seed", 1.5)])
def test_matcher_refuses_by_name(name, value):
    from laplace_amd.data.dataset import AdjList
    from laplace_amd.data.matching import RandomWalkMatcher
    u, a = WE.small_graph()
    users, articles = AdjList.from_edges(u, a, WE.N_USERS), AdjList.from_edges(a, u, WE.N_ITEMS)
    kw = dict(GOOD, k=5)
    kw[name] = value
    k = kw.pop("k")
    with pytest.raises(ValueError, match="num_walks" if value == 4097 else name):
        RandomWalkMatcher(users, articles, k, **kw)
    m = RandomWalkMatcher(users, articles, 5)
    assert (m.num_walks, m.walk_length, m.restart_prob, m.n_recent, m.boost, m.exclude_seen, m.seed) == (256, 4, 0.5, 8, "multi_hit", False, 0)
    for bad in (-1, WE.N_USERS, 1.0):
        with pytest.raises(ValueError, match="user_id"):
            m.get_matches(bad)
    with pytest.raises(ValueError, match="num_users"):
        m.matches_for_all_device(WE.N_USERS + 1, "cpu")


@pytest.mark.parametrize("name,value", BAD + [("seed", -1)])
def test_recommender_refuses_by_name(name, value):
    from laplace_amd.pinsage.evaluation import RandomWalkRecommender
    with pytest.raises(ValueError, match="num_walks" if value == 4097 else name):
        RandomWalkRecommender(**dict(GOOD, **{name: value}))


def test_recommender_refuses_k_graph_and_empty_users():
    from laplace_amd.pinsage.evaluation import RandomWalkRecommender
    rec = RandomWalkRecommender(**GOOD)
    ptr, idx = np.array([0, 2, 2, 3]), np.array([0, 1, 1])
    h = t.zeros(2, 4)
    for K in (0, -2):
        with pytest.raises(ValueError, match="k must be"):
            rec.recommend((ptr, idx), K, None, h)
    with pytest.raises(ValueError, match="at least one interaction"):
        rec.recommend((ptr, idx), 3, None, h)
    with pytest.raises(ValueError, match="h_item"):
        rec.recommend((ptr, idx), 3, None, None)
    with pytest.raises(ValueError, match="names item"):
        rec.recommend((np.array([0, 2, 3]), np.array([0, 1, 5])), 3, None, h)
    with pytest.raises(ValueError, match="num_walks"):       # 2048 * 4 visits
        RandomWalkRecommender(num_walks=2048)


# ---- the C entry: argument errors and the limit, nothing enqueued (no device here) -------------------------------------------
def test_c_entry_checks_arguments_before_any_launch():
    from laplace_amd import _lib
    L = _lib.lib()

    def call(n=4, k=5, W=8, Lw=2, p=0.5, n_recent=4, boost=0, exclude=0, ptrs=True, n_items=10):
        x = 4096 if ptrs else None            # an aligned non-null address: never read before the launch, and no launch happens
        return L.mi_match_random_walks_i32(n, None, 10, n_items, x, x, x, x, None, k, W, Lw, p, n_recent, boost, exclude, 1, 0,
                                           x, None, None, None)

    B, U = _lib.MI_ERR_BAD_ARG, _lib.MI_ERR_UNSUPPORTED
    assert call(ptrs=False) == B                                     # null pointers
    assert call(exclude=1) == B                                      # exclude_seen without the sorted rows
    for kw in (dict(k=0), dict(W=0), dict(Lw=-1), dict(p=1.0), dict(p=-0.5), dict(p=float("nan")), dict(n_recent=0), dict(n_recent=17),
               dict(boost=2), dict(n=-1)):
        assert call(**kw) == B, kw
        assert call(ptrs=False, **kw) == B, kw
    assert call(W=1025, Lw=4) == U and call(W=4097, Lw=1, ptrs=False) == U and call(W=1, Lw=4097) == U
    assert call(W=1024, Lw=4, ptrs=False) == B                       # at the limit: taken, and then refused for its pointers
    assert call(k=0, W=4097) == B                                    # an argument error comes before the limit
    assert call(n_items=2 ** 31 - 1) == _lib.MI_ERR_TOO_LARGE
    assert call(n=0, ptrs=False) == 0                                # zero queries: success, nothing enqueued
    assert _lib.MI_WALK_MATCH_MAX_VISITS == 4096 and _lib.MI_WALK_BOOSTS == {"sum": 0, "multi_hit": 1}
