"""GPU: the random-walk matcher (csrc/walk_match.hip: mi_match_random_walks_i32) against the numpy mirror of its rule
(tests/random_walk_matcher_emulation.py).  Integer counts, correctly rounded roots and one rounding per float operation: ids,
scores and counts are compared with ==, never to a tolerance.

The graph is tests/random_walk_matcher_emulation.small_graph: a shuffled log of 300 users x 90 items x 2 600 entries with
repeats, three empty users, an unsold item, a user whose only item nobody else holds, a user with 150 entries over 10 items and
a user with a row of 3 000 entries.  Ties abound at these sizes, so the id-ascending rule is exercised without staging it."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch as t

import random_walk_matcher_emulation as WE

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED, STEP = 11, 2
SPECIAL = list(WE.EMPTY_USERS) + [WE.LONE_USER, WE.DUP_USER, WE.LONG_USER]
WALKS = [(1, 1), (7, 3), (33, 5), (64, 2), (256, 4), (1024, 4)]       # the last is the 4096-visit limit


@pytest.fixture(scope="module")
def world():
    from laplace_amd import ops
    from laplace_amd.data.dataset import AdjList
    u, a = WE.small_graph()
    icsr, ucsr = WE.csr_pair(u, a, WE.N_USERS, WE.N_ITEMS)
    users, articles = AdjList.from_edges(u, a, WE.N_USERS), AdjList.from_edges(a, u, WE.N_ITEMS)
    to32 = lambda x: t.from_numpy(np.ascontiguousarray(x.astype(np.int32))).to(DEV)
    csr = (to32(articles.ptr), to32(articles.idx), to32(users.ptr), to32(users.idx))
    return SimpleNamespace(u=u, a=a, icsr=icsr, ucsr=ucsr, users=users, articles=articles, csr=csr,
                           ui_sorted=ops.sort_csr_rows(csr[2], csr[3]), counts={})


def _np(x):
    return tuple(y.cpu().numpy() for y in x)


def _mirror_counts(w, W, L, p, n_recent, users):
    """slot_counts of the listed users at (SEED, STEP), computed once per walk setting and shared (never changed)."""
    have = w.counts.setdefault((W, L, p, n_recent), {})
    rule = WE.Rule(W, L, p, n_recent, "sum", False)
    for u in users:
        if u not in have:
            have[u] = WE.slot_counts(u, w.icsr, w.ucsr, rule, SEED, STEP)
    return have


def test_sorted_rows_are_the_rows_sorted(world):
    got = world.ui_sorted.cpu().numpy()
    assert got.dtype == np.int32 and got.shape == world.users.idx.shape
    for u in (1, 2, WE.DUP_USER, WE.LONG_USER, WE.N_USERS - 1):
        assert np.array_equal(got[world.users.ptr[u]:world.users.ptr[u + 1]], np.sort(world.users[u]))


# ---- 1. the device equals the mirror -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_recent", [1, 3, 16])
@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("W,L", WALKS)
def test_device_equals_mirror(world, W, L, p, n_recent):
    """Crossed inside: both boosts x exclude_seen on / off x k in 1, 12, 200 (200 is more than the eligible items: pads)."""
    from laplace_amd import ops
    query = list(range(WE.N_USERS)) if W * L <= 512 else sorted(set(SPECIAL) | set(range(0, 300, 6)))
    q = t.tensor(query, dtype=t.int64, device=DEV)
    counts = _mirror_counts(world, W, L, p, n_recent, query)
    for boost in ("sum", "multi_hit"):
        for exclude_seen in (False, True):
            rule = WE.Rule(W, L, p, n_recent, boost, exclude_seen)
            want = [WE.match_user(u, world.icsr, world.ucsr, rule, 200, SEED, STEP, counts=counts[u]) for u in query]
            want_ids, want_sc = np.stack([x[0] for x in want]), np.stack([x[1] for x in want])
            want_cnt = np.array([x[2] for x in want], dtype=np.int32)
            assert (want_cnt < 200).all() and (W * L < 64 or want_cnt.max() > 12)      # k = 200 pads every row, k = 12 cuts some
            for k in (1, 12, 200):
                ids, sc, cnt = _np(ops.match_random_walks(*world.csr, k, num_walks=W, walk_length=L, restart_prob=p,
                                                          n_recent=n_recent, boost=boost, exclude_seen=exclude_seen, seed=SEED,
                                                          step=STEP, query_users=q, ui_sorted=world.ui_sorted))
                what = (boost, exclude_seen, k)
                assert ids.dtype == np.int32 and sc.dtype == np.float32 and cnt.dtype == np.int32 and ids.shape == (len(query), k)
                bad = np.flatnonzero((ids != want_ids[:, :k]).any(1) | (sc != want_sc[:, :k]).any(1) | (cnt != want_cnt))
                assert bad.size == 0, (what, [query[r] for r in bad[:5]], ids[bad[:1]], want_ids[bad[:1], :k])
            row = {u: r for r, u in enumerate(query)}
            for u in WE.EMPTY_USERS:                                    # an empty row: no proposal, and that is not an error
                assert (ids[row[u]] == -1).all() and (sc[row[u]] == 0).all() and cnt[row[u]] == 0
            assert (cnt[row[WE.LONE_USER]] == 0) == exclude_seen        # their only item leads back to themselves alone
            if not exclude_seen:
                assert ids[row[WE.LONE_USER], 0] == WE.LONE_ITEM


# ---- 2. who is asked, and how often, does not matter ---------------------------------------------------------------------------
KW = dict(num_walks=256, walk_length=4, restart_prob=0.5, n_recent=8, boost="multi_hit", exclude_seen=True, seed=SEED, step=STEP)


@pytest.fixture(scope="module")
def full(world):
    from laplace_amd import ops
    return tuple(x.clone() for x in ops.match_random_walks(*world.csr, 12, **KW))


def test_subset_permuted_and_repeated_queries_equal_the_full_rows(world, full):
    from laplace_amd import ops
    g = np.random.default_rng(3)
    sub = g.permutation(WE.N_USERS)[:120]
    sub[7] = sub[3]                                       # a repeated id
    sub[11], sub[12] = 299, WE.LONG_USER                  # an empty user, the long row
    for q in (t.from_numpy(sub).to(DEV), sub, sub.tolist()):     # ids on the device, and on the host (checked there)
        got = ops.match_random_walks(*world.csr, 12, query_users=q, **KW)
        for x, y in zip(got, full):
            assert t.equal(x, y[t.from_numpy(sub).to(DEV)])
    with pytest.raises(ValueError, match="query_users"):
        ops.match_random_walks(*world.csr, 12, query_users=[0, WE.N_USERS], **KW)
    # ids on the device are not read back: one outside the graph gets no proposal and touches nothing
    got = ops.match_random_walks(*world.csr, 12, query_users=t.tensor([5, WE.N_USERS, -1, 2 ** 40], device=DEV), **KW)
    assert t.equal(got[0][0], full[0][5]) and bool((got[0][1:] == -1).all()) and bool((got[2][1:] == 0).all())


def test_a_prefix_of_the_users_equals_the_full_rows(world, full):
    from laplace_amd import ops
    for n in (1, 100):
        got = ops.match_random_walks(*world.csr, 12, n_queries=n, **KW)
        for x, y in zip(got, full):
            assert x.shape[0] == n and t.equal(x, y[:n])
    got = ops.match_random_walks(*world.csr, 12, n_queries=0, **KW)
    assert got[0].shape == (0, 12) and got[2].shape == (0,)


def test_two_calls_give_equal_bits_and_seed_and_step_matter(world, full):
    from laplace_amd import ops
    again = ops.match_random_walks(*world.csr, 12, **KW)
    for x, y in zip(again, full):
        assert t.equal(x, y)
    no_sorted = ops.match_random_walks(*world.csr, 12, ui_sorted=None, **KW)     # the sorted rows built by the call itself
    assert all(t.equal(x, y) for x, y in zip(no_sorted, full))
    for other in (dict(seed=SEED + 1), dict(step=STEP + 1), dict(seed=SEED + 2 ** 32), dict(step=STEP + 2 ** 24)):
        got = ops.match_random_walks(*world.csr, 12, **dict(KW, **other))
        assert not t.equal(got[0], full[0]), other
        assert t.equal(got[0][list(WE.EMPTY_USERS)], full[0][list(WE.EMPTY_USERS)])


def test_4097_visits_are_refused(world):
    from laplace_amd import _lib, ops
    for W, L in ((4097, 1), (1025, 4), (1, 4097)):
        with pytest.raises(ValueError, match="num_walks"):
            ops.match_random_walks(*world.csr, 12, **dict(KW, num_walks=W, walk_length=L))
    iu_ptr, iu_idx, ui_ptr, ui_idx = world.csr
    out = t.full((4, 12), 7, dtype=t.int32, device=DEV)
    rc = _lib.lib().mi_match_random_walks_i32(4, None, WE.N_USERS, WE.N_ITEMS, iu_ptr.data_ptr(), iu_idx.data_ptr(), ui_ptr.data_ptr(),
                                              ui_idx.data_ptr(), None, 12, 1025, 4, 0.5, 8, 1, 0, SEED, STEP, out.data_ptr(), None,
                                              None, _lib.current_stream())
    t.cuda.synchronize()
    assert rc == _lib.MI_ERR_UNSUPPORTED and bool((out == 7).all())          # nothing was enqueued


# ---- 3. the layers above ------------------------------------------------------------------------------------------------------
def test_matcher_rows_equal_ops_rows(world, full):
    from laplace_amd.data.matching import RandomWalkMatcher
    kw = {k: v for k, v in KW.items() if k != "step"}
    m = RandomWalkMatcher(world.users, world.articles, 12, **kw)
    from laplace_amd import ops
    want = ops.match_random_walks(*world.csr, 12, **dict(KW, step=0))
    got = m.matches_for_all_device(WE.N_USERS, DEV)
    assert got.dtype == t.int64 and t.equal(got, want[0].long())
    ids, sc, cnt = m.matches_for_all_device(WE.N_USERS, DEV, with_scores=True)
    assert t.equal(ids, got) and t.equal(sc, want[1]) and t.equal(cnt, want[2])
    sub = t.tensor([WE.LONG_USER, 5, 5, 299], device=DEV)
    assert t.equal(m.matches_for_all_device(4, DEV, query_users=sub), got[sub])
    assert np.array_equal(m.matches_for_all(50), got[:50].cpu().numpy())
    for u in (5, 299, WE.LONE_USER, WE.LONG_USER):
        row = got[u].cpu()
        assert t.equal(m.get_matches(u), row[row >= 0])
    assert m._sorted is not None and m._on(DEV)[1].data_ptr() == m._sorted.data_ptr()          # the sorted rows are built once


def test_candidate_csr_device_is_the_row_wise_concatenation(world):
    from laplace_amd.data.device_sampler import candidate_csr_device
    from laplace_amd.data.matching import PopularItemsMatcher, RandomWalkMatcher
    ms = [PopularItemsMatcher.from_adjacency(world.articles, 10),
          RandomWalkMatcher(world.users, world.articles, 15, num_walks=64, walk_length=2, seed=SEED)]
    ptr, idx = candidate_csr_device(ms, WE.N_USERS, DEV)
    pop = ms[0].popular_items[:10].numpy()
    walks = ms[1].matches_for_all_device(WE.N_USERS, DEV).cpu().numpy()
    rows = [np.concatenate([pop, r[r >= 0]]) for r in walks]
    assert np.array_equal(ptr.cpu().numpy(), np.concatenate([[0], np.cumsum([len(r) for r in rows])]))
    assert np.array_equal(idx.cpu().numpy(), np.concatenate(rows))
    assert any(len(r) < 25 for r in rows) and any(len(r) == 25 for r in rows)                   # padded and full rows


def test_recommender_equals_the_matcher_and_evaluate_nn_takes_it():
    from laplace_amd.data.dataset import AdjList
    from laplace_amd.data.matching import RandomWalkMatcher
    from laplace_amd.pinsage.evaluation import RandomWalkRecommender, evaluate_nn, prec
    u, a = WE.small_graph()
    u = np.concatenate([u, WE.EMPTY_USERS])               # the recommender's contract refuses users without interactions
    a = np.concatenate([a, [1, 2, 3]])
    users, articles = AdjList.from_edges(u, a, WE.N_USERS), AdjList.from_edges(a, u, WE.N_ITEMS)
    kw = dict(num_walks=64, walk_length=3, restart_prob=0.5, n_recent=4, boost="multi_hit", seed=5)
    want = RandomWalkMatcher(users, articles, 10, exclude_seen=True, **kw).matches_for_all_device(WE.N_USERS, DEV)
    to32 = lambda x: t.from_numpy(x.astype(np.int32)).to(DEV)
    graph = SimpleNamespace(ui_ptr=to32(users.ptr), ui_idx=to32(users.idx), iu_ptr=to32(articles.ptr), iu_idx=to32(articles.idx))
    rec = RandomWalkRecommender(**kw)
    h = t.zeros(WE.N_ITEMS, 4, device=DEV)
    got = rec.recommend(graph, 10, None, h)
    assert got.dtype == t.int64 and got.shape == (WE.N_USERS, 10) and t.equal(got, want)
    assert t.equal(rec.recommend(graph, 10, None, t.randn(WE.N_ITEMS, 7, device=DEV)), want)    # the embeddings are ignored
    # a graph without item rows: they are derived, the users of an item in (user id, row position) order — the mirror on that
    icsr, ucsr = WE.csr_pair(u, a, WE.N_USERS, WE.N_ITEMS)
    by_user = np.argsort(u, kind="stable")
    icsr_t, _ = WE.csr_pair(u[by_user], a[by_user], WE.N_USERS, WE.N_ITEMS)
    derived = rec.recommend(users, 10, None, h).cpu().numpy()
    some = [0, 5, 150, WE.DUP_USER, WE.LONG_USER]
    mirror = WE.match(some, icsr_t, ucsr, WE.Rule(64, 3, 0.5, 4, "multi_hit", True), 10, seed=5)[0]
    assert np.array_equal(derived[some], mirror)
    with pytest.raises(ValueError, match="at least one interaction"):
        rec.recommend(AdjList.from_edges(*WE.small_graph(), WE.N_USERS), 10, None, h)
    # evaluate_nn: hits@K of the graph alone
    held = (np.arange(WE.N_USERS + 1), want[:, 3].clamp(min=0).cpu().numpy())       # every user's 4th recommendation is held out
    model = SimpleNamespace(item_representations=lambda sampler, step=None: h)
    hits = evaluate_nn(model, graph, held, K=10, recommender=rec)
    assert hits == prec(want, held) and hits > 0.9


# ---- 4. quality on the planted graph ---------------------------------------------------------------------------------------------
def test_recall_on_planted_graph_beats_popularity():
    """The Philox mirror on the CPU (tests/random_walk_matcher_emulation.match on this graph, these settings, seed 0) gives
    recall@12 = 0.325 exactly (325 of the 1000 held-out pairs; 0.336 at seed 1) against 0.171 for the 12 most popular items:
    1.90 x.  The device equals the mirror (the cases above), so the 1.3 x asked for (0.2223) is met by the reference alone; the
    margin covered nothing but the generator, which the numpy rehearsal (0.326-0.328) did not share."""
    from laplace_amd import synthetic as S
    from laplace_amd.data.dataset import AdjList
    from laplace_amd.data.matching import PopularItemsMatcher, RandomWalkMatcher
    spec = S.SyntheticSpec(2000, 600, 30000, seed=5, deg_min=2, deg_max=200, communities=8)
    ei = S.generate(spec)
    held = S.heldout_edges(spec, ei, 1000)
    eu, ea = ei[0].numpy(), ei[1].numpy()
    users, articles = AdjList.from_edges(eu, ea, spec.num_users), AdjList.from_edges(ea, eu, spec.num_items)
    m = RandomWalkMatcher(users, articles, 12, num_walks=1024, walk_length=4, restart_prob=0.5, n_recent=16, boost="multi_hit",
                          exclude_seen=True)
    got = m.matches_for_all_device(held.shape[1], DEV, query_users=held[0].to(DEV)).cpu()
    recall = float((got == held[1][:, None]).any(dim=1).float().mean())
    pop = PopularItemsMatcher.from_adjacency(articles, 12).get_matches(0)
    recall_pop = float(t.isin(held[1], pop).float().mean())
    print(f"recall@12: random walks {recall:.4f}, popular {recall_pop:.4f}")
    assert recall >= 1.3 * recall_pop, (recall, recall_pop)
